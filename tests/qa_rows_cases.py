"""Shared by tests/golden/make_golden_qa_rows.py, tests/test_qa_rows_host.py and tests/test_gpu_qa_rows.py: the cases of
the device-side ScanQA / SQA3D batch (sceneverse_amd/data/gpu_qa.py: qa_rows, csrc/gps_obj_select_qa.hip), a numpy
restatement of its rule and the emulation of its device law, both written from the statement in include/gps_hip.h.  The
fixture tests/golden/qa_rows_ref.npz holds only what the REFERENCE's own `ScanNetScanQAOld.__getitem__` and
`ScanNetSQA3D.__getitem__` made of the `ref` cases; the scans are regenerated here from seeds.

Every row is its own question about its own scan.  A 'gt' scan is its list of labels (rows_cases' generators; one point
per object); a 'pred' scan is pred_rows_cases' scene of 13 annotated cubes with proposals that are trimmed copies of them
(a copy at f >= 1/2 overlaps its cube at IoU >= 0.25 and takes its label, one at f <= 1/4 does neither).

What the cases contain, by construction (counted by `check_construction`):
  sizes     scans of 0, 1, 63, 64, 65, 130 and 1024 positions, 'gt' and 'pred'; 1025 in `ref=False` rows;
  M         2, 5 and 79 with O = M + 1, and O = M; n = M and n = M + 1;
  k         0, 1, 2 and 5 targets (k < M: what the reference runs), in list order that is not ascending; targets first,
            last and beyond position 64; two targets of one class and of two; a target that is a wall (appended: ref under
            filter_lang, ref=False without); class-mates numbering M - k - 1, M - k and M - k + 1; remained empty;
  labels    -100 and >= n_labels (ref=False); answers: A = 1, 65, 706, 8864, ids repeated, outside the vocabulary
            (ScanQA drops them, SQA3D maps them to 'u') and, ref=False, ids >= A;
  variants  1 and 3 per question, the reference's random.choice replayed; a per-variant keep (filter_lang);
  'pred'    a proposal that hits two targets (it carries the first one's label), targets nothing hits, no target at all,
            a tgt_label that differs from the object's own; SQA3D's raw labels;
  ref=False only the four definitions of include/gps_hip.h and out-of-range ids: an unkept target without filter_lang, a
            repeated target, k > M, empty rows."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pred_rows_cases as PC  # noqa: E402
import rows_cases as RC  # noqa: E402
from refer_cases import iou  # noqa: E402
from rows_cases import device_order  # noqa: E402,F401
from text_cases import M64, rng_u32  # noqa: E402

N_LABELS = 607                                   # sem_type '607'
INT2CAT = list(RC.INT2CAT) + [f"filler{i}" for i in range(len(RC.INT2CAT), N_LABELS)]
CAT2INT = {w: i for i, w in enumerate(INT2CAT)}
BACKGROUND = RC.BACKGROUND
MAX_SCAN, MAX_TGT, PAD_LABEL = 1024, 32, 5
SIZES = (0, 1, 63, 64, 65, 130, 1024)
MS = (2, 5, 79)
KS = (0, 1, 2, 5)
FG = RC.FG


def keep_fg():
    return np.asarray([c not in BACKGROUND for c in INT2CAT], dtype=bool)


# ---- rows ---------------------------------------------------------------------------------------------------------------
def _row(scan, tgt=(), answers=(), tgt_label=None, situations=("",), question="what is it ?", sqa_type=0):
    """scan: ('gt', labels) or ('pred', props of pred_rows_cases).  tgt: positions among the scan's annotated objects,
    in list order.  answers: ids; a negative one stands for an answer outside the vocabulary.  texts: the variants'
    strings situation_i + question (ScanQA: the question alone)."""
    return {"scan": scan, "tgt": [int(t) for t in tgt], "answers": [int(a) for a in answers],
            "tgt_label": None if tgt_label is None else [int(l) for l in tgt_label], "situations": list(situations),
            "question": question, "texts": [s + question for s in situations], "sqa_type": int(sqa_type)}


def scan_multi(n_fg, tgt_labels, n_mates, seed, n_bg=3, place=None):
    """n_fg foreground objects: one target per entry of tgt_labels, n_mates others whose label is one of those, the rest
    of other classes; n_bg background objects in between.  place: 'first' / 'last' puts the targets there, in REVERSED
    order (the list order is never ascending).  -> (labels, the targets' positions in list order)."""
    rng = np.random.default_rng(seed)
    k = len(tgt_labels)
    others = [c for c in FG if c not in tgt_labels]
    rest = n_fg - k - n_mates
    assert rest >= 0 and (k or not n_mates)
    body = [int(tgt_labels[i % k]) for i in range(n_mates)] + [int(c) for c in rng.choice(others, size=rest)]
    body += [int(c) for c in rng.integers(0, 3, size=n_bg)]
    body = [body[i] for i in rng.permutation(len(body))]
    at = {"first": [0] * k, "last": [len(body)] * k, None: sorted(int(x) for x in rng.integers(len(body) + 1, size=k))}[place]
    pos = []
    for i, a in enumerate(at):                   # insert from the left: an entry moves the later ones by one
        body.insert(a + i, None)
        pos.append(a + i)
    order = list(rng.permutation(k)) if place is None else list(range(k))[::-1]
    tgt = [pos[i] for i in order]
    for j, p in enumerate(tgt):
        body[p] = int(tgt_labels[j])
    return np.asarray(body, dtype=np.int32), tgt


def _answers(rng, A, kind):
    """kind 0: none; 1: one id; 2: two ids, one repeated; 3: ids with one outside the vocabulary (negative)."""
    ids = [int(a) for a in rng.integers(0, A, size=2)] + [A - 1, 0]
    return [[], ids[:1], [ids[0], ids[1], ids[0]], [ids[2], -100, ids[3]]][kind % 4]


def _tgt_labels(k):
    return [5, 7, 5, 9, 7][:k]                   # two classes from k = 2 on, a repeated class from k = 3 on


def _gt_rows(M, A, seed):
    """The ScanQA 'gt' rows for M objects per row; every one is a row the reference runs (k < M, targets kept)."""
    rng = np.random.default_rng(seed)
    ks = [k for k in KS if k < M]
    rows = []
    for i, n in enumerate(SIZES):                                               # sizes, k cycling
        labels, _ = RC.random_scan(n, 100 * M + n)
        fg = np.flatnonzero(labels >= 3)
        k = min(ks[i % len(ks)], len(fg))
        rows.append(_row(("gt", labels), rng.permutation(fg)[:k], _answers(rng, A, i)))
    for k in ks:
        tl = _tgt_labels(k)
        s = 1000 * M + 10 * k
        items = [scan_multi(M, tl, min(1, M - k) if k else 0, s + 1),             # n = M: no crop
                 scan_multi(M + 1, tl, 0, s + 2),                                  # n = M + 1: all but one of remained
                 scan_multi(M + 70, tl, 1 if k else 0, s + 3, n_bg=20, place="last"),   # targets last, beyond position 64
                 scan_multi(M + 6, tl, 1 if k else 0, s + 4, place="first")]
        if k:
            items += [scan_multi(M + 10, tl, M - k - 1, s + 5),                   # class-mates leave one slot
                      scan_multi(M + 10, tl, M - k, s + 6),                       # ... fill the row exactly
                      scan_multi(M + 10, tl, M - k + 1, s + 7),                   # ... are cut
                      scan_multi(M + 5, tl, M + 5 - k, s + 8)]                    # remained is empty
        if k == 2:
            items += [scan_multi(M + 10, [7, 7], 2, s + 9)]                      # two targets of ONE class
        rows += [_row(("gt", l), t, _answers(rng, A, j + k)) for j, (l, t) in enumerate(items)]
    return rows


def _sentences(rows, seed, n_var=0):
    """filter_lang: every variant's string names some foreground categories (never a wall: such a target is appended).
    n_var = 0: ScanQA, the names stand in the question; else SQA3D, n_var situations that name different ones."""
    rng = np.random.default_rng(seed)
    out = []
    for r in rows:
        named = [" ".join(INT2CAT[c] for c in FG if rng.random() < 0.6) for _ in range(max(n_var, 1))]
        if n_var:
            out.append(_row(r["scan"], r["tgt"], r["answers"], r["tgt_label"], [f"i face the {n} . " for n in named],
                            r["question"], r["sqa_type"]))
        else:
            out.append(_row(r["scan"], r["tgt"], r["answers"], r["tgt_label"], question=f"what is near the {named[0]} ?"))
    return out


SQA_QUESTIONS = ("what is there ?", "is it there ?", "how many ?", "can i sit ?", "which one ?", "where is it ?")   # types 0 .. 5


def _sqa_rows(M, A, seed, n_var=3):
    """SQA3D rows: never a target; 1 or n_var situations; answers outside the vocabulary become 'u' (the last id)."""
    rng = np.random.default_rng(seed)
    scans = [RC.random_scan(n, 300 * M + n)[0] for n in SIZES]
    scans += [scan_multi(M, [], 0, 17 * M + 1)[0], scan_multi(M + 1, [], 0, 17 * M + 2)[0], scan_multi(M + 10, [], 0, 17 * M + 3)[0]]
    rows = []
    for i, l in enumerate(scans):
        nv = 1 if i % 3 == 0 else n_var
        rows.append(_row(("gt", l), (), _answers(rng, A, i), situations=[f"situation {v} of row {i} . " for v in range(nv)],
                         question=SQA_QUESTIONS[i % 6], sqa_type=i % 6))
    return rows


# ---- 'pred' rows: proposals as trimmed copies of pred_rows_cases' annotated cubes ---------------------------------------
ANN_LABELS = PC.ANN_LABELS
S_SLAB, D_CUBE = 4, PC.D                         # they share their place: a proposal on D overlaps both


def pred_props(P, seed, tgt, hits=(), n_mates=0, tgt_label=None, extra=()):
    """P proposals: `hits` = positions that are a copy (f >= 1/2) of a target, by turns; n_mates further positions of a
    target's class -- by turns a low copy whose RAW label is that class and a copy of a PLAIN object of that class when
    there is one; the rest on PLAIN objects that are no target and of no target's class, any f, raw label likewise.
    extra: {position: (object, f, raw)} placed as given."""
    rng = np.random.default_rng(seed)
    tl = [ANN_LABELS[t] for t in tgt] if tgt_label is None else list(tgt_label)
    tl_all = set(tl) | {ANN_LABELS[t] for t in tgt}
    plain = [j for j in PC.PLAIN if j not in tgt and ANN_LABELS[j] not in tl_all]
    other_labels = [l for l in range(3, 12) if l not in tl_all]
    same = [j for j in PC.PLAIN if j not in tgt and ANN_LABELS[j] in set(tl)]
    extra = dict(extra)
    free = [p for p in range(P) if p not in hits and p not in extra]
    mates = set(int(p) for p in rng.permutation(free)[:n_mates])
    assert len(mates) == n_mates and (tgt or not hits)
    props, h = [], 0
    for p in range(P):
        if p in extra:
            props.append(extra[p])
        elif p in hits:
            props.append((tgt[h % len(tgt)], PC.FRACS[2 + int(rng.integers(3))], int(rng.integers(3, 12))))
            h += 1
        elif p in mates:
            if same and len(props) % 2:
                props.append((same[int(rng.integers(len(same)))], PC.FRACS[2 + int(rng.integers(3))], int(rng.integers(3, 12))))
            else:
                props.append((plain[int(rng.integers(len(plain)))], PC.FRACS[int(rng.integers(2))], tl[len(props) % len(tl)]))
        else:
            props.append((plain[int(rng.integers(len(plain)))], PC.FRACS[int(rng.integers(5))],
                          other_labels[int(rng.integers(len(other_labels)))]))
    return props


def _pred_rows(M, A, seed):
    """ScanQA 'pred' rows; the reference runs every one (fewer than M hits where P > M)."""
    rng = np.random.default_rng(seed)
    T2 = [9, 2]                                                                 # classes 9 and 7, list order not ascending
    rows = []
    for i, P in enumerate(SIZES):
        tgt = [[], [2], T2, [2, 3]][i % 4]
        k = min(len(tgt), M - 1, P)
        hits = tuple(int(x) for x in np.linspace(0, P - 1, k).astype(int)) if k else ()
        hits = tuple(sorted(set(hits))) if tgt else ()
        rows.append(_row(("pred", pred_props(P, 100 * M + P, tgt, hits, n_mates=min(P // 8, 2) if tgt else 0)), tgt,
                         _answers(rng, A, i)))
    s = 7 * M
    km = min(M - 1, 5)
    rows += [
        _row(("pred", pred_props(M, s + 1, [2], (M - 1,))), [2], _answers(rng, A, 1)),                       # P = M
        _row(("pred", pred_props(M + 1, s + 2, [2], (M,))), [2], _answers(rng, A, 2)),                       # P = M + 1
        _row(("pred", pred_props(M + 10, s + 3, [2], (4,), n_mates=M - 2)), [2], _answers(rng, A, 3)),       # mates leave one slot
        _row(("pred", pred_props(M + 10, s + 4, [2], (0,), n_mates=M - 1)), [2], _answers(rng, A, 0)),       # ... fill the row
        _row(("pred", pred_props(M + 10, s + 5, [2], (M + 9,), n_mates=M)), [2], _answers(rng, A, 1)),       # ... are cut
        _row(("pred", pred_props(M + 5, s + 6, [2], (2,), n_mates=M + 4)), [2], _answers(rng, A, 2)),        # remained is empty
        _row(("pred", pred_props(M + 300, s + 7, T2, tuple(range(5, 5 + 70 * km, 70))[:km], n_mates=1)), T2,
             _answers(rng, A, 3)),                                                                          # hits beyond 64 / 256
        _row(("pred", pred_props(M + 20, s + 8, [2], ())), [2], _answers(rng, A, 0)),                        # a target nothing hits
        _row(("pred", pred_props(M + 20, s + 9, [], ())), [], _answers(rng, A, 1)),                          # no target at all
        _row(("pred", pred_props(M + 20, s + 10, [2], (3,), n_mates=1, tgt_label=[8])), [2], _answers(rng, A, 2),
             tgt_label=[8]),                                                                                # cat2int[object_name] differs
        # one proposal (a copy of D) overlaps BOTH the slab and D: it carries the label of whichever comes first
        _row(("pred", pred_props(M + 12, s + 11, [S_SLAB, D_CUBE], (), extra={1: (D_CUBE, 1.0, 9)})), [S_SLAB, D_CUBE],
             _answers(rng, A, 3)),
        _row(("pred", pred_props(M + 12, s + 12, [D_CUBE, S_SLAB], (), extra={M + 3: (D_CUBE, 0.75, 9)})), [D_CUBE, S_SLAB],
             _answers(rng, A, 0)),
    ]
    return rows


def _sqa_pred_rows(M, A, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for i, P in enumerate((0, 1, M, M + 1, 65, 130)):
        rows.append(_row(("pred", pred_props(P, 500 * M + P, [], ())), (), _answers(rng, A, i),
                         situations=[f"situation {v} . " for v in range(1 + 2 * (i % 2))], question=SQA_QUESTIONS[2], sqa_type=2))
    return rows


def _case(name, M, O, A, rows, kind="scanqa", pc_type="gt", lang=False, ref=True, seed=0):
    """kind 'scanqa': float32 multi-hots, matched labels, one variant; 'sqa3d': int64, raw labels, the variant drawn."""
    return {"name": name, "M": M, "O": O, "A": A, "rows": rows, "kind": kind, "pc_type": pc_type, "lang": lang, "ref": ref,
            "seed": seed}


def build_cases():
    A_OF = {2: 65, 5: 706, 79: 8864}
    cases = [_case(f"qa_gt_M{M}", M, M + 1, A_OF[M], _gt_rows(M, A_OF[M], 11 * M), seed=31 * M) for M in MS]
    cases.append(_case("qa_gt_M5_O5", 5, 5, 1, _gt_rows(5, 1, 57), seed=41))
    rows = _gt_rows(5, 65, 58)
    wall = [_row(("gt", l), [t]) for l, t in (RC.crafted(5, 0, 71, tgt_wall=True, place="first"),      # n = M + 1, the wall last
                                             RC.crafted(4, 0, 72, tgt_wall=True),                    # n = M: the wall in the last slot
                                             RC.crafted(30, 0, 73, tgt_wall=True))]
    cases.append(_case("qa_gt_M5_lang", 5, 6, 65, _sentences(rows + wall, 5), lang=True, seed=47))
    cases.append(_case("sqa_gt_M5", 5, 6, 706, _sqa_rows(5, 706, 61), kind="sqa3d", seed=53))
    cases.append(_case("sqa_gt_M79", 79, 80, 65, _sqa_rows(79, 65, 62), kind="sqa3d", seed=59))
    cases.append(_case("sqa_gt_M5_lang", 5, 6, 65, _sentences(_sqa_rows(5, 65, 63), 6, n_var=3), kind="sqa3d", lang=True, seed=61))
    cases += [_case(f"qa_pred_M{M}", M, M + 1, A_OF[M], _pred_rows(M, A_OF[M], 13 * M), pc_type="pred", seed=37 * M) for M in MS]
    cases.append(_case("qa_pred_M5_O5", 5, 5, 65, _pred_rows(5, 65, 77)[7:], pc_type="pred", seed=67))
    cases.append(_case("sqa_pred_M5", 5, 6, 706, _sqa_pred_rows(5, 706, 64), kind="sqa3d", pc_type="pred", seed=71))
    # ---- what the reference cannot run: the four definitions and out-of-range ids -----------------------------------------
    odd = []
    for l, t in (RC.crafted(5, 0, 81, tgt_wall=True, place="first"), RC.crafted(30, 2, 82, tgt_wall=True)):
        odd.append(_row(("gt", l), [t], [3]))                                   # an unkept target WITHOUT filter_lang
    l, t = scan_multi(20, [5, 7], 2, 83)
    odd.append(_row(("gt", l), [t[0], t[1], t[0], t[1], t[0]], [1]))            # repeated targets
    l, t = scan_multi(5, [5, 7], 0, 84)
    odd.append(_row(("gt", l), [t[1], t[1], t[0]], [2]))                        # ... uncropped
    l, t = scan_multi(30, [5, 7, 5, 9, 7, 8, 6], 3, 85)
    odd.append(_row(("gt", l), t, [4]))                                         # k = 7 > M
    l, t = scan_multi(30, [5, 7, 5, 9, 7], 3, 86)
    odd.append(_row(("gt", l), t, [5]))                                         # k = M
    for n, s in ((70, 2), (200, 3)):                                            # labels -100 and >= n_labels
        l, _ = RC.random_scan(n, 500 + s, p_bg=0.1)
        l[::4], l[1::7], l[2::9], l[3::11] = -100, N_LABELS, 100000, -1
        ok = np.flatnonzero((l >= 3) & (l < N_LABELS))
        odd.append(_row(("gt", l), [ok[len(ok) // 2], ok[0]], [6]))
    l, _ = RC.random_scan(20, 504)
    l[5] = -100
    odd.append(_row(("gt", l), [5], [7]))                                       # the target's own label is not valid
    odd.append(_row(("gt", RC.random_scan(40, 505)[0]), [], [64, 65, 70, 1000000, 0]))   # answer ids >= A
    odd.append(_row(("gt", RC.random_scan(1025, 506)[0]), [7], [8]))            # a scan over the cap
    cases.append(_case("qa_gt_M5_odd", 5, 6, 65, odd, ref=False, seed=73))
    oddp = [_row(("pred", pred_props(40, 901, [2], tuple(range(1, 40, 4)))), [2], [1]),              # k = 10 > M
            _row(("pred", pred_props(300, 902, [9, 2], (0, 63, 64, 255, 256))), [9, 2], [2]),        # k = M
            _row(("pred", pred_props(1025, 903, [2], (3, 700))), [2], [3]),                          # a scan over the cap
            _row(("pred", pred_props(30, 904, [2, 2, 9], (3, 9))), [2, 2, 9], [4])]                  # a repeated target
    cases.append(_case("qa_pred_M5_odd", 5, 6, 65, oddp, pc_type="pred", ref=False, seed=79))
    return cases


CASES = build_cases()
CASE_IDS = [c["name"] for c in CASES]
REF_CASES = [c for c in CASES if c["ref"]]
REF_IDS = [c["name"] for c in REF_CASES]


def scene_id(case, b):
    return f"{case['name']}-{b}"


def answer_ids(case, row):
    """What the caller's vocabulary makes of the row's answers: ScanQA keeps an answer outside it as a negative id (which
    add_question drops), SQA3DAnswer.stoi maps it to 'u', the last id here."""
    if case["kind"] == "sqa3d":
        return [a if a >= 0 else case["A"] - 1 for a in row["answers"]]
    return list(row["answers"])


def keep_of(case):
    """The case's keep table: (n_labels,) bool, or with `lang` one row per variant of the whole case, in row order."""
    if not case["lang"]:
        return keep_fg()
    return np.stack([keep_fg() & np.asarray([c in text for c in INT2CAT]) for r in case["rows"] for text in r["texts"]], 0)


def var_first(case):
    first = np.zeros(len(case["rows"]) + 1, np.int64)
    np.cumsum([len(r["texts"]) for r in case["rows"]], out=first[1:])
    return first


def share_without_reference():
    n = sum(len(c["rows"]) for c in CASES)
    return sum(len(c["rows"]) for c in CASES if not c["ref"]) / n, n


# ---- the rule -----------------------------------------------------------------------------------------------------------
def device_pick(seed, b, n_var):
    return int(rng_u32((int(seed) + 4) & M64, np.uint64(b))) % n_var if n_var else 0


def restate_row(case, row, keep, order=None):
    """One row by the statement of include/gps_hip.h.  keep: the (n_labels,) table of the row's chosen variant ('gt').
    order: a sequence (replay) or a callable n_rem -> sequence.
    -> None for an EMPTY row, else dict(row = positions (-1 for a bad order entry), slots, n_rem, n_tgt, labels)."""
    M = case["M"]
    pred = case["pc_type"] == "pred"
    matched = case["kind"] == "scanqa"
    scan = row["scan"][1]
    n_ann = len(PC.ANN) if pred else len(scan)
    P = len(scan)
    raw = row["tgt"][:MAX_TGT]
    if P > MAX_SCAN or any(not 0 <= t < n_ann for t in raw):
        return None
    own = ANN_LABELS if pred else scan
    T, TL = [], []
    for j, t in enumerate(raw):                  # a repeated entry counts once, at its first place
        if t not in T:
            T.append(t)
            TL.append(int(own[t]) if row["tgt_label"] is None else row["tgt_label"][j])
    if pred:
        cls = [PC.matched_label(*q) if matched else q[2] for q in scan]
        sel, tg, tl = list(range(P)), [], []
        for p, (o, f, _) in enumerate(scan):
            for t, l in zip(T, TL):
                if iou(PC.prop_box(o, f), PC._ANN_BOXES[t]) >= 0.25:
                    tg.append(p)
                    tl.append(l)
                    break
    else:
        cls = [int(l) for l in scan]
        sel = [p for p, l in enumerate(cls) if 0 <= l < len(keep) and keep[l]]
        sel += [t for t in T if t not in sel]
        tg, tl = T, TL
    k, n, n_rem = len(tg), len(sel), 0
    if n <= M:
        out, slots = list(sel), [sel.index(t) for t in tg]
    else:
        kr = min(k, M)
        out, slots = list(tg[:kr]), list(range(kr))
        out = (out + [p for p in sel if p not in tg and cls[p] in tl])[:M]
        tl = tl[:kr]
        if len(out) < M:
            remained = [p for p in sel if p not in tg and cls[p] not in tl]
            n_rem = len(remained)
            o = order(n_rem) if callable(order) else order
            for j in range(M - len(out)):
                i = int(o[j])
                out.append(remained[i] if 0 <= i < n_rem else -1)
    return {"row": out, "slots": slots, "n_rem": n_rem, "n_tgt": len(slots), "labels": tl if k else [PAD_LABEL], "k": k,
            "obj_labels": [cls[p] if p >= 0 else -100 for p in out]}


def restate_case(case, order=None, pick=None, seed=None, offsets=None, text_ids=None):
    """The whole batch -> dict of arrays in the launch's layout (the multi-hots as uint8 0 / 1).  order (B, R), pick (B):
    replays; else the device law at `seed` (the pick is drawn for 'sqa3d' cases, the first variant otherwise).
    offsets: the global id of each row's first position (default 0).  text_ids: per variant of the case its text id
    (default: the variant's number)."""
    B, M, O, A = len(case["rows"]), case["M"], case["O"], case["A"]
    keep, vf = keep_of(case), var_first(case)
    out = {"row_obj": np.full((B, O), -1, np.int32), "n_sel": np.zeros(B, np.int32), "n_rem": np.zeros(B, np.int32),
           "n_tgt": np.zeros(B, np.int32), "sent_idx": np.full(B, -1, np.int32), "sqa_type": np.zeros(B, np.int64),
           "obj_labels": np.full((B, O), -100, np.int64), "tgt_object_id": np.zeros((B, O), np.uint8),
           "tgt_object_label": np.zeros((B, N_LABELS), np.uint8), "answer_label": np.zeros((B, A), np.uint8)}
    for b, row in enumerate(case["rows"]):
        nv = len(row["texts"])
        if pick is not None:
            pk = int(pick[b])
        else:
            pk = device_pick(seed, b, nv) if case["kind"] == "sqa3d" else 0
        pk = pk if 0 <= pk < nv else 0
        v = int(vf[b]) + pk
        o = order[b] if order is not None else (lambda n, b=b: device_order(seed, b, n))
        r = restate_row(case, row, keep[v] if keep.ndim == 2 else keep, o)
        if r is None:
            continue
        sel = np.asarray(r["row"], dtype=np.int64)
        first = 0 if offsets is None else int(offsets[b])
        out["row_obj"][b, :len(sel)] = np.where(sel >= 0, sel + first, -1)
        out["n_sel"][b], out["n_rem"][b], out["n_tgt"][b] = len(sel), r["n_rem"], r["n_tgt"]
        out["sent_idx"][b] = v if text_ids is None else int(text_ids[v])
        out["sqa_type"][b] = row["sqa_type"]
        out["obj_labels"][b, :len(sel)] = r["obj_labels"]
        for s in (r["slots"] if r["k"] else [len(sel)]):
            if s < O:
                out["tgt_object_id"][b, s] = 1
        for l in r["labels"]:
            if 0 <= l < N_LABELS:
                out["tgt_object_label"][b, l] = 1
        for a in answer_ids(case, row):
            if 0 <= a < A:
                out["answer_label"][b, a] = 1
    return out


OUT_KEYS = ("row_obj", "n_sel", "n_rem", "n_tgt", "sqa_type", "obj_labels", "tgt_object_id", "tgt_object_label", "answer_label")


def check_construction():
    """What the module's docstring promises, counted on the restatement."""
    share, n_rows = share_without_reference()
    assert share <= 0.25, share
    seen = {"gt": set(), "pred": set()}
    ks, n_vars, As = set(), set(), set()
    facts = set()
    for case in CASES:
        M, keep, vf = case["M"], keep_of(case), var_first(case)
        As.add(case["A"])
        for b, row in enumerate(case["rows"]):
            seen[case["pc_type"]].add(len(row["scan"][1]))
            n_vars.add(len(row["texts"]))
            r = restate_row(case, row, keep[int(vf[b])] if keep.ndim == 2 else keep, lambda n: np.arange(n))
            if r is None:
                facts.add("empty")
                continue
            if case["ref"]:
                ks.add(r["k"])
                assert r["k"] < M or len(r["row"]) <= M and r["n_rem"] == 0 and r["k"] <= M, (case["name"], b)
                assert len(set(row["tgt"])) == len(row["tgt"]), (case["name"], b)
            n = len(r["row"])
            if r["n_rem"] == 0 and n == M:
                facts.add("full without a fill")
            if r["k"] >= 2 and r["slots"] != sorted(r["slots"]):
                facts.add("slots not ascending")
            if any(t > 64 for t in row["tgt"]):
                facts.add("beyond 64")
            if case["pc_type"] == "pred" and row["tgt"] and r["k"] == 0:
                facts.add("nothing hits")
    assert set(SIZES) | {1025} <= seen["gt"] and set(SIZES) | {1025} <= seen["pred"], seen
    assert set(KS) <= ks and {1, 3} <= n_vars and {1, 65, 706, 8864} <= As, (ks, n_vars, As)
    assert {"empty", "full without a fill", "slots not ascending", "beyond 64", "nothing hits"} <= facts, facts
    # the proposal on D carries the label of whichever of the slab and D comes first in the list
    case = next(c for c in CASES if c["name"] == "qa_pred_M5")
    a, b2 = (restate_row(case, r, None, lambda n: np.arange(n)) for r in case["rows"][-2:])
    assert a["labels"] == [ANN_LABELS[S_SLAB]] and b2["labels"] == [ANN_LABELS[D_CUBE]] and a["k"] == b2["k"] == 1
    return share, n_rows


# ---- packing ------------------------------------------------------------------------------------------------------------
def gt_scene(labels):
    """A 'gt' scan as add_scan takes it: one point per object."""
    n = len(labels)
    pts = np.zeros((n, 3), np.float32)
    pts[:, 0] = np.arange(n)
    return pts, np.zeros((n, 3), np.uint8), np.arange(n), list(range(n)), [int(l) for l in labels]


def pack(cases=None, device="cpu"):
    """Every row's scan of `cases` as its own scan of one PackedScans (id = scene_id), finalized, and every row as its own
    question of one PackedQuestions (variant v of a case's text ids: 7 * v + 3 past the earlier cases').
    -> (packed, questions, {case name: (first question, text ids of its variants)})."""
    from sceneverse_amd.data import gpu_objects as G
    from sceneverse_amd.data.gpu_qa import PackedQuestions
    cases = CASES if cases is None else cases
    packed, questions = G.PackedScans(device), PackedQuestions(device)
    for case in cases:
        for b, row in enumerate(case["rows"]):
            sid = scene_id(case, b)
            if case["pc_type"] == "pred":
                s = PC.make_scene(row["scan"][1])
                packed.add_scan(sid, s["points"], s["colors"], s["instance_labels"], s["inst_ids"], inst_labels=s["inst_labels"])
                packed.add_proposals(sid, s["points"], s["colors"], s["masks"], s["prop_labels"])
            else:
                pts, col, inst, ids, labels = gt_scene(row["scan"][1])
                packed.add_scan(sid, pts, col, inst, ids, inst_labels=labels)
    packed.finalize()
    where, n_text = {}, 0
    for case in cases:
        first, ids = questions.n_questions, []
        for b, row in enumerate(case["rows"]):
            texts = [7 * (n_text + v) + 3 for v in range(len(row["texts"]))]
            n_text += len(texts)
            ids += texts
            questions.add_question(scene_id(case, b), row["tgt"], answer_ids(case, row), texts, row["tgt_label"], row["sqa_type"])
        where[case["name"]] = (first, np.asarray(ids, dtype=np.int64))
    return packed, questions.finalize(packed), where
