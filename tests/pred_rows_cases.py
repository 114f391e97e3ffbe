"""Shared by tests/golden/make_golden_pred_rows.py, tests/test_pred_rows_host.py and tests/test_gpu_pred_rows.py: the
cases of the device-side selection of PREDICTED proposals (sceneverse_amd/data/gpu_objects.py: select_rows(pc_type=
"pred"), csrc/gps_obj_select_pred.hip), a numpy restatement of its rule and the emulation of its device law, both written
from the statement in include/gps_hip.h.  The fixture tests/golden/pred_rows_ref.npz holds only what the REFERENCE's own
`ScanBase._getitem_refer` made of the `ref` cases; the scenes are regenerated here from seeds.

Every scene has the same 13 annotated objects (ANN): unit cubes side by side whose clouds hold the two extreme corners
and, on the dyadic planes z = 1/8, 1/4, 1/2, 3/4, the corner points of the trimmed box -- so every box is exact.  Two
cubes (D, C2) share their place with a SLAB of half their height that comes FIRST in scan order and has another label: a
proposal on such a cube overlaps both and must take the slab's label (D's proposals JOIN class 7 that way, C2's LEAVE
it).  A proposal is a mask over the scene's points: the points of one cube with z <= f, f dyadic -- a trimmed copy at
volume fraction exactly f, IoU with its cube f / (1 + 1e-8): f = 1/4 and 1/2 fall just BELOW the two thresholds.

What the cases contain, by construction (asserted by `check_construction`):
  P         0, 1, 63, 64, 65, 130 and 1024 proposals; 1025 in a `ref=False` row;
  M         2, 5 and 79 with O = M + 1, and O = M; P = M and P = M + 1;
  pinned    blocks of 0 (uncropped), 1, 3 and M - 1 proposals, members on both sides of position 64 and of position
            256; the pair (3, 9), whose CPython set order is 9, 3;
  nested    proposals on the target at f = 1/4 (not pinned) and 1/2 (pinned at 0.25, not flagged at 0.5);
  classes   M - 2, M - 1 and M class-mates by MATCHED label; every unpinned proposal of the target's class (remained is
            empty); mates that join the class through a slab, and one that leaves it;
  label_map a map that merges two labels; a tgt_label that differs from the target's own label;
  ref=False no hit with P > M, k > M, k = M, a target outside its scan, a scan of 1025 proposals."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from refer_cases import CAT2INT, INT2CAT, box_of, iou  # noqa: E402,F401
from rows_cases import device_order  # noqa: E402,F401
from text_cases import M64, rng_u32  # noqa: E402,F401

N_LABELS = len(INT2CAT)
MAX_SCAN = 1024
SIZES = (0, 1, 63, 64, 65, 130, 1024)
MS = (2, 5, 79)
DYADIC = (0.125, 0.25, 0.5, 0.75)
FRACS = DYADIC + (1.0,)
MERGE_MAP = np.asarray([0, 1, 2, 3, 4, 4, 6, 7, 8, 9, 10, 11], dtype=np.int32)     # label 5 counts as 4

# (place along x, height, label) in scan order.  T = 2 is the usual target; C is of its class; S / S2 are the slabs
ANN = ((0, 1.0, 3), (1, 1.0, 4), (2, 1.0, 7), (3, 1.0, 7), (4, 0.5, 7), (4, 1.0, 5), (5, 0.5, 6), (5, 1.0, 7),
       (6, 1.0, 8), (7, 1.0, 9), (8, 1.0, 5), (9, 1.0, 10), (10, 1.0, 0))
ANN_LABELS = [a[2] for a in ANN]
PLAIN = (0, 1, 2, 3, 8, 9, 10, 11, 12)           # cubes that share their place with nothing
T, C, D, C2 = 2, 3, 5, 7
INST0 = 100                                      # instance id of annotated object j is INST0 + j


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _points():
    """The points of the 13 annotated objects, the same in every scene: -> (points f32, instance ids)."""
    rng = np.random.default_rng(4242)
    pts, inst = [], []
    for j, (place, h, _) in enumerate(ANN):
        x0 = 2.0 * place
        p = [(x0, 0, 0), (x0 + 1, 1, h)]
        for f in DYADIC:
            if f < h:
                p += [(x0, 0, f), (x0 + 1, 1, f)]
        free = rng.random((6, 3)) * (1, 1, h) + (x0, 0, 0)
        p = np.concatenate([np.asarray(p, dtype=np.float64), free], 0).astype(np.float32)
        pts.append(p)
        inst.append(np.full(len(p), INST0 + j, dtype=np.int64))
    pts, inst = np.concatenate(pts, 0), np.concatenate(inst)
    perm = rng.permutation(len(pts))
    return pts[perm], inst[perm]


POINTS, INST = _points()
COLORS = np.random.default_rng(4243).integers(0, 256, size=(len(POINTS), 3)).astype(np.uint8)


def make_scene(props):
    """props: [(annotated object, f, raw label)] -> the scene in refer_cases' layout."""
    props = list(props)
    obj = np.asarray([q[0] for q in props], dtype=np.int64).reshape(-1, 1)
    f = np.asarray([q[1] for q in props], dtype=np.float32).reshape(-1, 1)
    masks = (INST[None, :] == INST0 + obj) & (POINTS[None, :, 2] <= f)
    return {"points": POINTS, "colors": COLORS, "instance_labels": INST, "inst_ids": [INST0 + j for j in range(len(ANN))],
            "inst_labels": list(ANN_LABELS), "masks": masks.reshape(len(props), len(POINTS)),
            "prop_labels": [int(q[2]) for q in props], "props": props}


def crafted(P, seed, t=T, pins=(), n_mates=0, lt=None, extra=()):
    """P proposals for target t: `pins` = the positions that hit the target (f in 1/2, 3/4, 1), n_mates further
    positions of the target's class -- by turns an object of that class at f >= 1/2 (matched), D at f >= 1/2 when the
    class is S's (joins through the slab), and a low trimmed copy whose RAW label is the class (unmatched) -- and the rest
    of other classes.  extra: {position: (object, f, raw)} placed as given.  lt: the class when it is not t's label."""
    rng = np.random.default_rng(seed)
    lt = ANN_LABELS[t] if lt is None else lt
    others = [l for l in range(3, N_LABELS) if l != lt]
    matched = [j for j in PLAIN if ANN_LABELS[j] == lt and j != t] + ([D] if lt == ANN_LABELS[4] else [])
    extra = dict(extra)
    free = [p for p in range(P) if p not in pins and p not in extra]
    mates = set(int(p) for p in rng.permutation(free)[:n_mates])
    assert len(mates) == n_mates
    props = []
    for p in range(P):
        if p in extra:
            props.append(extra[p])
        elif p in pins:
            props.append((t, FRACS[2 + int(rng.integers(3))], int(rng.integers(3, N_LABELS))))
        elif p in mates:
            kind = len(props) % 3
            if matched and kind != 2:
                props.append((matched[int(rng.integers(len(matched)))], FRACS[2 + int(rng.integers(3))],
                              int(rng.integers(3, N_LABELS))))
            else:
                props.append((PLAIN[int(rng.integers(len(PLAIN)))], FRACS[int(rng.integers(2))], lt))
        else:
            j = PLAIN[int(rng.integers(len(PLAIN)))]
            low = j == t or ANN_LABELS[j] == lt
            fr = FRACS[int(rng.integers(2))] if low else FRACS[int(rng.integers(5))]
            props.append((j, fr, others[int(rng.integers(len(others)))]))
    return props


def _row(props, t=T, tgt_label=None):
    return {"props": props, "tgt": t, "tgt_label": tgt_label}


def _rows(M):
    """The 'refer' rows for M proposals per row; every one is a row the reference runs."""
    k_some = min(3, M - 1)
    rows = []
    for P in SIZES:                                                             # sizes; cropped ones pin 1 .. 3
        pins = tuple(range(0, P, max(P // k_some, 1)))[:k_some] if P > M else tuple(range(0, P, 7))[:4]
        rows.append(_row(crafted(P, 100 * M + P, pins=pins, n_mates=min(P // 8, max(M - k_some - 1, 0), 2))))
    rows += [_row(crafted(M, 7 * M + 1, pins=(M - 1,), n_mates=min(1, M - 1))),             # P = M: no crop
             _row(crafted(M, 7 * M + 12)),                                                  # ... and no hit at all
             _row(crafted(M + 1, 7 * M + 2, pins=(M,))),                                    # P = M + 1: all but one of remained
             _row(crafted(M + 10, 7 * M + 3, pins=(4,), n_mates=M - 2)),                    # class-mates leave one slot
             _row(crafted(M + 10, 7 * M + 4, pins=(0,), n_mates=M - 1)),                    # ... fill the row exactly
             _row(crafted(M + 10, 7 * M + 5, pins=(M + 9,), n_mates=M)),                    # ... are cut
             _row(crafted(M + 5, 7 * M + 6, pins=(2,), n_mates=M + 4)),                     # remained is empty
             _row(crafted(M + 300, 7 * M + 7, pins=(1, 70, 299 + M)[:k_some], n_mates=2)),  # both sides of 64 and 256
             _row(crafted(M + 300, 7 * M + 8, pins=tuple(range(5, 5 + 4 * (M - 1), 4)), n_mates=3)),   # M - 1 pinned
             _row(crafted(M + 20, 7 * M + 9, t=0, pins=(M + 3,), n_mates=1), t=0),             # a target alone in its class
             _row(crafted(M + 20, 7 * M + 10, t=10, pins=(3,), n_mates=2), t=10),
             _row(crafted(M + 20, 7 * M + 15, t=1, pins=(2,), n_mates=1), t=1)]              # class 4: alone unless 5 counts as 4               # class 5: D and object 10
    # nested at exactly 1/4 and 1/2; D joins class 7 through the slab S, C2 (raw label 7 too) leaves it through S2
    extra = {0: (T, 0.25, 4), 2: (T, 0.5, 4), 5: (D, 0.75, 9), 6: (C2, 0.75, 7), 8: (C2, 1.0, 7), 11: (D, 0.5, 7)}
    rows.append(_row(crafted(M + 12, 7 * M + 11, pins=(2,), extra=extra)))
    if M >= 5:                                                                  # the pair whose set order is 9, 3
        rows.append(_row(crafted(M + 30, 7 * M + 13, pins=(3, 9), n_mates=1)))
        rows.append(_row(crafted(M + 30, 7 * M + 14, pins=(3, 9, 65), n_mates=M)))
    return rows


def _case(name, M, O, rows, label_map=None, ref=True, seed=0):
    return {"name": name, "M": M, "O": O, "rows": rows, "label_map": label_map, "ref": ref, "seed": seed}


def build_cases():
    cases = [_case(f"pred_M{M}", M, M + 1, _rows(M), seed=31 * M) for M in MS]
    cases.append(_case("pred_M5_O5", 5, 5, _rows(5)[7:], seed=41))
    cases.append(_case("pred_M5_map", 5, 6, _rows(5)[7:], label_map=MERGE_MAP, seed=43))
    rows = [_row(r["props"], r["tgt"], tgt_label=l) for r, l in zip(_rows(5)[7:], (8, 7, 3, 9, 7, 8, 7, 5, 4, 7, 10, 7, 3, 6, 7))]
    cases.append(_case("pred_M5_tgtlabel", 5, 6, rows, seed=47))
    # ---- what the reference cannot run ---------------------------------------------------------------------------------
    odd = [_row(crafted(40, 901)),                                              # no hit with P > M
           _row(crafted(40, 902, pins=tuple(range(1, 40, 4)))),                 # k = 10 > M
           _row(crafted(300, 903, pins=(0, 63, 64, 255, 256))),                 # k = M, on the segment boundaries
           _row(crafted(40, 904, pins=(3,)), t=len(ANN)),                       # a target one past its scan
           _row(crafted(40, 905, pins=(3,)), t=-1),                             # ... before it
           _row(crafted(1025, 906, pins=(3, 700))),                             # a scan over the cap
           _row(crafted(1024, 907)),                                            # the cap itself without a hit
           _row(crafted(20, 908, pins=(3,)), tgt_label=N_LABELS)]               # a class outside the label list
    cases.append(_case("pred_M5_odd", 5, 6, odd, label_map=MERGE_MAP, ref=False, seed=59))
    return cases


CASES = build_cases()
CASE_IDS = [c["name"] for c in CASES]
REF_CASES = [c for c in CASES if c["ref"]]
REF_IDS = [c["name"] for c in REF_CASES]


def scene_id(case, b):
    return f"{case['name']}-{b}"


# ---- the rule --------------------------------------------------------------------------------------------------------
_ANN_BOXES = [box_of(POINTS[INST == INST0 + j]) for j in range(len(ANN))]
_PROP_BOX = {}


def prop_box(obj, f):
    if (obj, f) not in _PROP_BOX:
        _PROP_BOX[(obj, f)] = box_of(POINTS[(INST == INST0 + obj) & (POINTS[:, 2] <= np.float32(f))])
    return _PROP_BOX[(obj, f)]


_MATCH = {}


def matched_label(obj, f, raw):
    """base.py:359-366: the label of the FIRST annotated object that overlaps the proposal by >= 0.25, else its own."""
    if (obj, f) not in _MATCH:
        b = prop_box(obj, f)
        _MATCH[(obj, f)] = next((ANN_LABELS[j] for j, g in enumerate(_ANN_BOXES) if iou(g, b) >= 0.25), None)
    m = _MATCH[(obj, f)]
    return raw if m is None else m


def restate_row(row, M, O, label_map=None, order=None):
    """One row by the statement of include/gps_hip.h.  order: a sequence (replay) or a callable n_rem -> sequence.
    -> dict(row = positions (-1 for a bad order entry), tgt_slot, n_rem, is_multiple, is_hard, iou25 (O), iou50 (O),
    tgt_id, labels (O))."""
    props, t = row["props"], row["tgt"]
    P = len(props)
    res = {"row": [], "tgt_slot": -1, "n_rem": 0, "is_multiple": False, "is_hard": False}
    if 0 <= t < len(ANN) and P <= MAX_SCAN:
        l_t = ANN_LABELS[t] if row["tgt_label"] is None else int(row["tgt_label"])
        v = [iou(prop_box(o, f), _ANN_BOXES[t]) for o, f, _ in props]
        m = [matched_label(*q) for q in props]
        h25 = [x >= 0.25 for x in v]
        pinned = [p for p in range(P) if h25[p]]
        if P <= M:
            sel = list(range(P))
        elif len(pinned) >= M:
            sel = pinned[len(pinned) - M:]
        else:
            sel = (pinned + [p for p in range(P) if not h25[p] and m[p] == l_t])[:M]
            if len(sel) < M:
                remained = [p for p in range(P) if not h25[p] and m[p] != l_t]
                res["n_rem"] = len(remained)
                o = order(len(remained)) if callable(order) else order
                for k in range(M - len(sel)):
                    i = int(o[k])
                    sel.append(remained[i] if 0 <= i < len(remained) else -1)
        res["row"] = sel
        if pinned:
            res["tgt_slot"] = max(s for s, p in enumerate(sel) if p >= 0 and h25[p])
        if 0 <= l_t < N_LABELS:
            lm = np.arange(N_LABELS) if label_map is None else np.asarray(label_map)
            res["is_multiple"] = sum(lm[l] == lm[l_t] for l in ANN_LABELS) > 1
            res["is_hard"] = sum(l == l_t for l in ANN_LABELS) > 2
    sel = res["row"]
    f25, f50, lab = np.zeros(O, np.int64), np.zeros(O, np.int64), np.full(O, -100, np.int64)
    for s, p in enumerate(sel):
        if p >= 0:
            f25[s], f50[s], lab[s] = v[p] >= 0.25, v[p] >= 0.5, m[p]
    res.update(iou25=f25, iou50=f50, labels=lab,
               tgt_id=res["tgt_slot"] if res["tgt_slot"] >= 0 else sum(p >= 0 for p in sel))
    return res


def restate_case(case, order=None, seed=None, offsets=None):
    """The whole batch -> dict of arrays in the launch's layout.  order (B, R): replay; else the device law at `seed`.
    offsets: the global id of each row's first proposal (default 0: positions)."""
    B, M, O = len(case["rows"]), case["M"], case["O"]
    out = {"row_obj": np.full((B, O), -1, np.int32), "tgt_slot": np.zeros(B, np.int32), "n_sel": np.zeros(B, np.int32),
           "n_rem": np.zeros(B, np.int32), "is_multiple": np.zeros(B, bool), "is_hard": np.zeros(B, bool),
           "iou25": np.zeros((B, O), np.int64), "iou50": np.zeros((B, O), np.int64), "tgt_id": np.zeros(B, np.int64),
           "labels": np.zeros((B, O), np.int64)}
    for b in range(B):
        o = order[b] if order is not None else (lambda n, b=b: device_order(seed, b, n))
        r = restate_row(case["rows"][b], M, O, case["label_map"], o)
        row = np.asarray(r["row"], dtype=np.int64)
        first = 0 if offsets is None else int(offsets[b])
        out["row_obj"][b, :len(row)] = np.where(row >= 0, row + first, -1)
        out["n_sel"][b] = len(row)
        for k in ("tgt_slot", "n_rem", "is_multiple", "is_hard", "iou25", "iou50", "tgt_id", "labels"):
            out[k][b] = r[k]
    return out


def compare_with_reference(mine, ref, b, M):
    """Row b of a restated (or launched) batch against the reference's, both with POSITIONS in row_obj / sel, under the
    comparison of include/gps_hip.h: the pinned block as a set, everything else exactly.  -> list of what differs."""
    bad = []
    sel_m, sel_r = mine["row_obj"][b], ref["sel"][b]
    n = int(ref["n_sel"][b])
    if int(mine["n_sel"][b]) != n or (sel_m[n:] != -1).any():
        return ["n_sel"]
    for k in ("n_rem", "is_multiple", "is_hard"):
        if mine[k][b] != ref[k][b]:
            bad.append(k)
    if not np.array_equal(mine["iou25"][b], ref["iou25"][b]):
        bad.append("iou25 (bit for bit)")
    k25 = int(ref["iou25"][b].sum())
    cropped = ref["n_rem"][b] > 0 or not np.array_equal(sel_r[:n], np.arange(n))
    head = k25 if cropped else 0
    if set(sel_m[:head].tolist()) != set(sel_r[:head].tolist()):
        bad.append("pinned block as a set")
    if not np.array_equal(sel_m[head:n], sel_r[head:n]):
        bad.append("row behind the block")
    tm, tr = int(mine["tgt_id"][b]), int(ref["tgt_id"][b])
    if k25 == 0:
        if tm != n or tr != n:
            bad.append("tgt_id without a hit")
    elif sel_m[tm] != sel_r[tr]:
        bad.append("object in tgt_object_id's slot")
    if set(sel_m[:n][mine["iou50"][b][:n] != 0].tolist()) != set(sel_r[:n][ref["iou50"][b][:n] != 0].tolist()):
        bad.append("objects flagged at 0.5")
    if mine["iou50"][b][n:].any() or ref["iou50"][b][n:].any():
        bad.append("iou50 past the row")
    if dict(zip(sel_m[:n].tolist(), mine["labels"][b][:n].tolist())) != dict(zip(sel_r[:n].tolist(), ref["labels"][b][:n].tolist())):
        bad.append("obj_labels per object")
    if (mine["labels"][b][n:] != -100).any():
        bad.append("obj_labels past the row")
    return bad


# ---- the end-to-end batch: logits that are a function of the PROPOSAL ------------------------------------------------------
E2E_CASE = "pred_M5"


def e2e_rows():
    """Rows of E2E_CASE with more proposals than a row holds (batch_rows refuses them), of moderate size."""
    case = next(c for c in CASES if c["name"] == E2E_CASE)
    return [b for b, r in enumerate(case["rows"]) if case["M"] < len(r["props"]) <= 400]


def pinned_positions(row):
    return [p for p, (o, f, _) in enumerate(row["props"]) if iou(prop_box(o, f), _ANN_BOXES[row["tgt"]]) >= 0.25]


def proposal_scores(case, b):
    """(P,) float32, one score per proposal of row b: normal draws; every third row favours its LAST pinned proposal (the
    target id's), the next a pinned proposal at f = 1/2 (a hit at 0.25 only) or else its FIRST one, and the third has all
    its pinned proposals pushed below the rest (a miss)."""
    row = case["rows"][b]
    x = np.random.default_rng(7000 + 31 * case["seed"] + b).standard_normal(len(row["props"])).astype(np.float32)
    pinned = pinned_positions(row)
    if pinned and b % 3 == 0:
        x[pinned[-1]] = 8.0
    elif pinned and b % 3 == 1:
        half = [p for p in pinned if row["props"][p][1] == 0.5]
        x[half[0] if half else pinned[0]] = 8.0
    elif pinned:
        x[pinned] = -8.0
    return x


def slot_logits(case, rows, sel):
    """(len(rows), O) float32: the proposals' scores placed into slots by the row table `sel` of POSITIONS, -inf in the
    padding slots."""
    out = np.full(sel.shape, -np.inf, dtype=np.float32)
    for i, b in enumerate(rows):
        x = proposal_scores(case, b)
        real = sel[i] >= 0
        out[i, real] = x[sel[i][real]]
    return out


def check_construction():
    """What the module's docstring promises, counted on the restatement."""
    seen_P, seen_k = set(), {M: set() for M in MS}
    for case in CASES:
        M = case["M"]
        for row in case["rows"]:
            P = len(row["props"])
            seen_P.add(P)
            if case["ref"]:
                r = restate_row(row, M, case["O"], case["label_map"], lambda n: np.arange(n))
                k = int(r["iou25"].sum())
                assert P <= M or 1 <= k < M, (case["name"], P, k)       # the reference runs it
                if case["name"] == f"pred_M{M}":
                    seen_k[M].add(k if P > M else -k)
    assert set(SIZES) | {1025} <= seen_P, seen_P
    for M in MS:
        assert {1, min(3, M - 1), M - 1} <= seen_k[M] and 0 in seen_k[M], (M, seen_k[M])
        rows = CASES[MS.index(M)]["rows"]
        full = [restate_row(r, M, M + 1, None, lambda n: np.arange(n)) for r in rows]
        assert any(len(r["props"]) == M for r in rows) and any(len(r["props"]) == M + 1 for r in rows)
        assert any(len(r["props"]) > M and f["n_rem"] == 0 and len(f["row"]) == M for r, f in zip(rows, full))   # mates fill / cut
        assert any(len(r["props"]) > M and f["n_rem"] == 0 and int((np.asarray(f["row"]) >= 0).sum()) == M and
                   len(r["props"]) == M + 5 for r, f in zip(rows, full))               # remained is empty
    r = restate_row(CASES[1]["rows"][-3], 5, 6, None, lambda n: np.arange(n))   # the nested / join / leave row of M = 5
    assert r["iou25"][:1].tolist() == [1] and r["iou50"][0] == 0                # pinned at exactly 1/2: not flagged at 0.5
    assert matched_label(D, 0.75, 9) == 7 and matched_label(C2, 0.75, 7) == 6 and matched_label(T, 0.25, 4) == 4


# ---- packing -----------------------------------------------------------------------------------------------------------
def pack(cases=None, device="cpu"):
    """Every row's scene of `cases` as its own scan of one PackedScans (id = scene_id), finalized."""
    from sceneverse_amd.data import gpu_objects as G
    packed = G.PackedScans(device)
    for case in (CASES if cases is None else cases):
        for b, row in enumerate(case["rows"]):
            s = make_scene(row["props"])
            sid = scene_id(case, b)
            packed.add_scan(sid, s["points"], s["colors"], s["instance_labels"], s["inst_ids"], inst_labels=s["inst_labels"])
            packed.add_proposals(sid, s["points"], s["colors"], s["masks"], s["prop_labels"])
    return packed.finalize()
