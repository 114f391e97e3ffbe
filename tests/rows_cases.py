"""Shared by tests/golden/make_golden_rows.py, tests/test_rows_host.py and tests/test_gpu_rows.py: the cases of the
device-side object selection (sceneverse_amd/data/gpu_objects.py: select_rows, csrc/gps_obj_select.hip), a numpy
restatement of its rule and the emulation of its device law, both written from the statement in include/gps_hip.h.

A scan is its list of labels (the selection reads nothing else), regenerated from the case's seeds; the fixture
tests/golden/rows_ref.npz holds only what the REFERENCE's own `_getitem_refer`, `_getitem_pretrain` and
`_getitem_obj_pretrain` made of them.  Cases the reference cannot run (a label outside the category list, a target outside
its scan, a scan over the cap) are `ref=False`: the kernel is compared with the restatement alone there.

What the cases contain, by construction:
  sizes     scans of 0, 1, 63, 64, 65, 130 and 1024 positions (wave and block boundaries of the kernel);
  M         2, 5 and 79 objects per row with O = M + 1 slots, and O = M;
  crafted   n = M (no crop) and n = M + 1 (the fill takes all but one of remained); the target first, last, a wall that is
            appended last, beyond position 64; M - 2, M - 1 and M class-mates of the target; every foreground object of
            the target's class (remained is empty);
  labels    -100 and labels >= n_labels (never kept, never counted); a label_map that merges two labels;
  keep      one batch with a per-row table (filter_lang), one with the CLASS_LABELS_200 filter.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from text_cases import M64, rng_u32  # noqa: E402

# three names outside CLASS_LABELS_200 at the end: the `only=` filter of _getitem_obj_pretrain drops them
INT2CAT = ["wall", "floor", "ceiling", "chair", "table", "door", "couch", "cabinet", "shelf", "desk", "thingamajig", "whatsit"]
IN_200 = INT2CAT[:10]
BACKGROUND = ("wall", "floor", "ceiling")
N_LABELS = len(INT2CAT)
FG = tuple(range(3, N_LABELS))
MAX_SCAN = 1024
SIZES = (0, 1, 63, 64, 65, 130, 1024)
MS = (2, 5, 79)
MERGE_MAP = np.asarray([0, 1, 2, 3, 4, 4, 6, 7, 8, 9, 10, 11], dtype=np.int32)     # door counts as table


def keep_fg():
    return np.asarray([c not in BACKGROUND for c in INT2CAT], dtype=bool)


def keep_200():
    return np.asarray([c not in BACKGROUND and c in IN_200 for c in INT2CAT], dtype=bool)


# ---- scans ----------------------------------------------------------------------------------------------------------
def random_scan(n, seed, p_bg=0.15):
    """n labels: foreground classes uniformly, about p_bg of them background; -> (labels, a foreground position or 0)."""
    rng = np.random.default_rng(seed)
    l = rng.choice(FG, size=n).astype(np.int32)
    bg = rng.random(n) < p_bg
    l[bg] = rng.integers(0, 3, size=int(bg.sum()))
    fg = np.flatnonzero(l >= 3)
    t = int(fg[rng.integers(len(fg))]) if len(fg) else 0
    return l, t


def crafted(n_fg, n_mates, seed, n_bg=3, tgt_label=5, place=None, tgt_wall=False):
    """n_fg foreground objects: the target (label tgt_label), n_mates others of its label, the rest of other classes;
    n_bg background objects in between.  tgt_wall: the target is one MORE object, a wall.  place: 'first' / 'last' puts
    the target at that position.  -> (labels, target position)."""
    rng = np.random.default_rng(seed)
    others = [c for c in FG if c != tgt_label]
    rest = n_fg - n_mates - (0 if tgt_wall else 1)
    assert rest >= 0
    body = [tgt_label] * n_mates + [int(c) for c in rng.choice(others, size=rest)] + [int(c) for c in rng.integers(0, 3, size=n_bg)]
    body = [body[i] for i in rng.permutation(len(body))]
    t_label = 0 if tgt_wall else tgt_label
    at = {"first": 0, "last": len(body), None: int(rng.integers(len(body) + 1))}[place]
    body.insert(at, t_label)
    return np.asarray(body, dtype=np.int32), at


def _refer_items(M):
    """(labels, target) of the 'refer' batch for M objects per row."""
    items = [random_scan(n, 100 * M + n) for n in SIZES if n >= 1]
    items += [crafted(M, min(1, M - 1), 7 * M + 1),                          # n = M: no crop
              crafted(M + 1, 0, 7 * M + 2),                                  # n = M + 1: all but one of remained
              crafted(M + 10, max(M - 2, 0), 7 * M + 3),                     # class-mates leave one slot
              crafted(M + 10, M - 1, 7 * M + 4),                             # ... fill the row exactly
              crafted(M + 10, M, 7 * M + 5),                                 # ... are cut
              crafted(M + 5, M + 4, 7 * M + 6),                              # every foreground object of one class
              crafted(M + 6, 1, 7 * M + 7, place="first"),
              crafted(M + 6, 1, 7 * M + 8, place="last"),
              crafted(M, 0, 7 * M + 9, tgt_wall=True, place="first"),         # n = M + 1, the wall appended last
              crafted(M - 1, 0, 7 * M + 10, tgt_wall=True),                   # n = M: the wall in the last slot
              crafted(M + 70, 3, 7 * M + 11, n_bg=20, place="last")]          # the target beyond position 64
    l, _ = random_scan(130, 9 * M)                                           # ... and a class-mate beyond it, target kept
    t = int(np.flatnonzero(l >= 3)[-1])
    items.append((l, t))
    return items


def _pretrain_items(M):
    items = [(random_scan(n, 200 * M + n)[0], -1) for n in SIZES]
    items += [(crafted(M, 0, 11 * M + 1)[0], -1), (crafted(M + 1, 0, 11 * M + 2)[0], -1)]
    return items


def _case(name, mode, M, O, items, keep="fg", label_map=None, ref=True, seed=0):
    return {"name": name, "mode": mode, "M": M, "O": O, "scans": [np.asarray(i[0], dtype=np.int32) for i in items],
            "tgt": [int(i[1]) for i in items], "keep": keep, "label_map": label_map, "ref": ref, "seed": seed}


def _sentences(n_rows, seed):
    """filter_lang: per row the category names its sentence mentions."""
    rng = np.random.default_rng(seed)
    return [" ".join(INT2CAT[c] for c in FG if rng.random() < 0.6) for _ in range(n_rows)]


def build_cases():
    cases = []
    for M in MS:
        cases.append(_case(f"refer_M{M}", "refer", M, M + 1, _refer_items(M), seed=31 * M))
        cases.append(_case(f"pretrain_M{M}", "pretrain", M, M, _pretrain_items(M), seed=37 * M))
    cases.append(_case("refer_M5_O5", "refer", 5, 5, _refer_items(5)[6:12], seed=41))
    cases.append(_case("refer_M79_map", "refer", 79, 80, _refer_items(79)[:9], label_map=MERGE_MAP, seed=43))
    items = _refer_items(5)
    cases.append(_case("refer_M5_lang", "refer", 5, 6, items, keep=_sentences(len(items), 5), seed=47))
    cases.append(_case("objpretrain_M5", "pretrain", 5, 5, _pretrain_items(5), keep="200", seed=53))
    # ---- what the reference cannot run ---------------------------------------------------------------------------------
    odd = []
    for n, s in ((9, 1), (70, 2), (200, 3)):
        l, t = random_scan(n, 500 + s, p_bg=0.1)
        l[::4] = -100
        l[1::7] = N_LABELS
        l[2::9] = 1000
        l[3::11] = -1
        ok = np.flatnonzero((l >= 3) & (l < N_LABELS))
        odd.append((l, int(ok[len(ok) // 2])))
    l, _ = random_scan(20, 504)
    l[5] = -100
    odd.append((l, 5))                                                       # the target's own label is not valid
    odd.append((np.zeros(0, np.int32), 0))                                   # a target outside its (empty) scan
    odd.append((random_scan(12, 505)[0], 12))                                # ... one past the end
    odd.append((random_scan(12, 506)[0], -1))                                # ... before the start
    cases.append(_case("refer_M5_odd", "refer", 5, 6, odd, label_map=MERGE_MAP, ref=False, seed=59))
    cases.append(_case("pretrain_M5_odd", "pretrain", 5, 7, [(o[0], -1) for o in odd], ref=False, seed=61))
    return cases


CASES = build_cases()
CASE_IDS = [c["name"] for c in CASES]
REF_CASES = [c for c in CASES if c["ref"]]
REF_IDS = [c["name"] for c in REF_CASES]


def keep_of(case):
    """The case's keep table: (n_labels,) bool, or (B, n_labels) for a per-row one."""
    k = case["keep"]
    if isinstance(k, str):
        return keep_fg() if k == "fg" else keep_200()
    return np.stack([keep_fg() & np.asarray([c in s for c in INT2CAT]) for s in k], 0)


# ---- the rule --------------------------------------------------------------------------------------------------------
def restate_row(labels, t, M, mode, keep, label_map=None, order=None):
    """One row.  labels: the scan; t: the target position (ignored in 'pretrain' mode); keep (n_labels,) bool;
    order: a sequence (the replay form) or a callable n_rem -> sequence (the device law).
    -> dict(row=[positions, -1 for a bad order entry], tgt_slot, n_rem, is_multiple, is_hard)."""
    labels = np.asarray(labels, dtype=np.int64)
    n_labels = len(keep)
    refer = mode == "refer"
    empty = {"row": [], "tgt_slot": -1, "n_rem": 0, "is_multiple": False, "is_hard": False}
    if len(labels) > MAX_SCAN or (refer and not 0 <= t < len(labels)):
        return empty
    valid = (labels >= 0) & (labels < n_labels)
    kept = valid.copy()
    kept[valid] = np.asarray(keep, dtype=bool)[labels[valid]]
    sel = [int(p) for p in np.flatnonzero(kept)]
    res = dict(empty)
    if refer:
        if t not in sel:
            sel.append(t)
        l_t = int(labels[t])
        if valid[t]:
            m = np.arange(n_labels) if label_map is None else np.asarray(label_map)
            res["is_multiple"] = bool((m[labels[valid]] == m[l_t]).sum() > 1)
            res["is_hard"] = bool((labels[valid] == l_t).sum() > 2)
    if len(sel) <= M:
        res["row"] = sel
        res["tgt_slot"] = sel.index(t) if refer else -1
        return res
    if refer:
        row = ([t] + [p for p in sel if p != t and labels[p] == l_t])[:M]
        remained = [p for p in sel if labels[p] != l_t]
        res["tgt_slot"] = 0
    else:
        row, remained = [], sel
    if len(row) < M:
        res["n_rem"] = len(remained)
        o = order(len(remained)) if callable(order) else order
        for k in range(M - len(row)):
            i = int(o[k])
            row.append(remained[i] if 0 <= i < len(remained) else -1)
    res["row"] = row
    return res


def device_order(seed, b, n_rem):
    """The device law: indices into remained in ascending order of (rng_u32(S + 3, b * 2^20 + r) << 32) | r."""
    r = np.arange(n_rem, dtype=np.uint64)
    h = rng_u32((int(seed) + 3) & M64, np.uint64(b) * np.uint64(1 << 20) + r)
    return np.argsort((h << np.uint64(32)) | r, kind="stable")


def restate_case(case, order=None, seed=None, offsets=None):
    """The whole batch -> dict of arrays in the launch's layout.  order (B, R): replay; else the device law at `seed`.
    offsets: the global id of each row's first object (default 0: scene-local positions)."""
    B, M, O = len(case["scans"]), case["M"], case["O"]
    keep = keep_of(case)
    out = {"row_obj": np.full((B, O), -1, np.int32), "tgt_slot": np.zeros(B, np.int32), "n_sel": np.zeros(B, np.int32),
           "n_rem": np.zeros(B, np.int32), "is_multiple": np.zeros(B, bool), "is_hard": np.zeros(B, bool)}
    for b in range(B):
        o = order[b] if order is not None else (lambda n, b=b: device_order(seed, b, n))
        r = restate_row(case["scans"][b], case["tgt"][b], M, case["mode"], keep if keep.ndim == 1 else keep[b],
                        case["label_map"], o)
        row = np.asarray(r["row"], dtype=np.int64)
        first = 0 if offsets is None else int(offsets[b])
        out["row_obj"][b, :len(row)] = np.where(row >= 0, row + first, -1)
        out["n_sel"][b] = len(row)
        for k in ("tgt_slot", "n_rem", "is_multiple", "is_hard"):
            out[k][b] = r[k]
    return out


def fill_ranks(seed, n_rows, n_rem):
    """(n_rows, n_rem) the place each object of remained takes under the device law, rows 0 .. n_rows - 1."""
    r = np.arange(n_rem, dtype=np.uint64)[None, :]
    b = np.arange(n_rows, dtype=np.uint64)[:, None]
    h = rng_u32((int(seed) + 3) & M64, b * np.uint64(1 << 20) + r)
    order = np.argsort((h << np.uint64(32)) | r, axis=1, kind="stable")
    ranks = np.empty_like(order)
    np.put_along_axis(ranks, order, np.broadcast_to(np.arange(n_rem), order.shape), axis=1)
    return ranks
