"""Scenes, batches and the float64 restatement for the ScanRefer target path (sceneverse_amd/data/gpu_objects.py:
add_proposals / refer_targets, engine.ScanReferCounter).  The scenes are regenerated from seeds; the fixture
tests/golden/refer_ref.npz (tests/golden/make_golden_refer.py) holds only what the REFERENCE's own
`ScanBase._getitem_refer`, `pad_tensors` and `ScanReferEval.batch_metrics` made of them.

What the scenes contain, by construction:
  small   annotated A (a slab, 40 % of B's box, FIRST in scan order) and B in the same place: the proposal that is all
          of B overlaps both at >= 0.25 and must take A's label (first match, not best match); T with points on exact
          dyadic coordinates and proposals nested in its box at volume ratios exactly 1/4 and 1/2 (IoU just below the
          thresholds because of the 1e-8), two more proposals on T at about 0.9 and 0.65 (the LAST one is the target id;
          they share points with each other and with the nested ones); a wall (dropped by the 'gt' selection); C with
          T's label (-> is_multiple); D that no proposal reaches (target id = n_b); an instance id without points and
          an empty mask (both skipped).  7 proposals: with O = 8 the reference's n_b + 1 flags just fit.
  big     20 annotated objects, 79 proposals = trimmed copies at about 0.2 / 0.45 / 0.7 / 0.95 of object p % 20: the
          hits of a target lie in slots j + 20, j + 40, j + 60, on both sides of slot 64 (the wave boundary).
  empty   3 annotated objects and no proposal at all (n_b = 0)."""
import numpy as np

INT2CAT = ["wall", "floor", "ceiling"] + [f"cat{i}" for i in range(3, 12)]
CAT2INT = {w: i for i, w in enumerate(INT2CAT)}


def _cloud(rng, lo, hi, n, extra=()):
    """n float32 points uniform in [lo, hi], the two extreme corners among them so that the box is exactly [lo, hi]."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    p = (rng.random((n, 3)) * (hi - lo) + lo).astype(np.float32)
    p = np.clip(p, lo.astype(np.float32), hi.astype(np.float32))
    fixed = [lo, hi] + [np.asarray(e, dtype=np.float64) for e in extra]
    p[:len(fixed)] = np.asarray(fixed, dtype=np.float32)
    return p


def _assemble(rng, objects, inst_order):
    """objects: {inst_id: (points, label)} -> shuffled scene arrays; inst_order may name ids without points."""
    pts = np.concatenate([objects[i][0] for i in objects], 0)
    inst = np.concatenate([np.full(len(objects[i][0]), i, dtype=np.int64) for i in objects])
    perm = rng.permutation(len(pts))
    pts, inst = pts[perm], inst[perm]
    colors = rng.integers(0, 256, size=(len(pts), 3)).astype(np.uint8)
    return {"points": pts, "colors": colors, "instance_labels": inst, "inst_ids": list(inst_order)}


def scene_small():
    rng = np.random.default_rng(11)
    t_extra = [(3, 5, 0.25), (3, 5, 0.5)]
    objects = {
        3: (_cloud(rng, (0, 0, 0), (1, 1, 0.4), 300), 5),                       # A
        7: (_cloud(rng, (0, 0, 0), (1, 1, 1), 700), 6),                         # B
        2: (_cloud(rng, (2, 4, 0), (3, 5, 1), 900, t_extra), 7),                # T, dyadic
        9: (_cloud(rng, (5, 0, 0), (5.125, 3, 2), 400), 0),                     # a wall
        4: (_cloud(rng, (0, 3, 0), (1, 4, 1), 500), 7),                         # C, T's class
        5: (_cloud(rng, (6, 6, 0), (7, 7, 1), 350), 8),                         # D
    }
    s = _assemble(rng, objects, [3, 7, 11, 2, 9, 4, 5])                         # 11 has no points
    s["inst_labels"] = [5, 6, 3, 7, 0, 7, 8]
    p, inst = s["points"], s["instance_labels"]
    masks = [inst == 7,
             (inst == 2) & (p[:, 0] <= 2.9),
             np.zeros(len(p), dtype=bool),
             (inst == 2) & (p[:, 2] <= 0.25),
             (inst == 2) & (p[:, 2] <= 0.5),
             (inst == 2) & (p[:, 0] >= 2.35),
             (inst == 4) & (p[:, 1] <= 3.6),
             (inst == 5) & (p[:, 0] <= 6.1)]
    s["masks"] = np.stack(masks, 0)
    s["prop_labels"] = [9, 10, 4, 11, 3, 10, 9, 4]
    return s


def scene_big():
    rng = np.random.default_rng(12)
    objects = {100 + j: (_cloud(rng, (2 * j, 0, 0), (2 * j + 1, 1, 1), 120 + 7 * j), 3 + j % 9) for j in range(20)}
    s = _assemble(rng, objects, [100 + j for j in range(20)])
    s["inst_labels"] = [3 + j % 9 for j in range(20)]
    p, inst = s["points"], s["instance_labels"]
    fracs = (0.2, 0.45, 0.7, 0.95)
    masks = []
    for q in range(79):
        j, f = q % 20, fracs[q // 20]
        masks.append((inst == 100 + j) & (p[:, 2] <= f))
    s["masks"] = np.stack(masks, 0)
    s["prop_labels"] = [3 + (q * 5) % 9 for q in range(79)]
    return s


def scene_empty():
    rng = np.random.default_rng(13)
    objects = {j + 1: (_cloud(rng, (j, j, 0), (j + 1, j + 2, 1), 64 + j), 4 + j) for j in range(3)}
    s = _assemble(rng, objects, [1, 2, 3])
    s["inst_labels"] = [4, 5, 6]
    s["masks"] = np.zeros((0, len(s["points"])), dtype=bool)
    s["prop_labels"] = []
    return s


_SCENES = {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = {"small": scene_small, "big": scene_big, "empty": scene_empty}[name]()
    return _SCENES[name]


SCENE_NAMES = ("small", "big", "empty")

# (name, O, pc_type, logits seed, items); item = (scene, referred instance id, slot the logits favour on even rows)
CASES = [
    ("pred8", 8, "pred", 21, [("small", 2, 4), ("small", 5, 6), ("small", 7, 0), ("small", 3, 0), ("small", 4, 5),
                              ("empty", 2, 0), ("small", 2, 2), ("small", 2, 1)]),
    ("pred80", 80, "pred", 22, [("big", 100, 60), ("big", 103, 63), ("big", 104, 64), ("big", 110, 70), ("big", 118, 78),
                                ("big", 119, 59), ("small", 2, 4), ("empty", 1, 0), ("big", 104, 44), ("big", 110, 10)]),
    ("gt8", 8, "gt", 23, [("small", 2, 2), ("small", 9, 5), ("small", 5, 4), ("empty", 3, 2), ("small", 4, 3),
                          ("small", 3, 0)]),
    ("gt80", 80, "gt", 24, [("big", 100, 0), ("big", 119, 19), ("small", 7, 1), ("big", 107, 7), ("empty", 1, 0),
                            ("big", 112, 12)]),
]
CASE_IDS = [c[0] for c in CASES]
METRIC_KEYS = ("og_acc_iou25", "og_acc_iou50", "og_acc_iou25_unique", "og_acc_iou50_unique", "og_acc_iou25_multiple",
               "og_acc_iou50_multiple", "og_acc")


def kept(s):
    """(inst ids, labels) of the instances the loader keeps: those with points, in inst_ids order (base.py:83-90)."""
    ids, labels = [], []
    for i, l in zip(s["inst_ids"], s["inst_labels"]):
        if np.any(s["instance_labels"] == i):
            ids.append(i)
            labels.append(l)
    return ids, labels


def gt_selection(s, target_inst):
    """selected_obj_idxs of the 'gt' branch without filter_lang (base.py:380-383): walls, floors and ceilings go,
    the target stays (appended last when it is one of them)."""
    ids, labels = kept(s)
    sel = [i for i, l in enumerate(labels) if INT2CAT[l] not in ("wall", "floor", "ceiling")]
    t = ids.index(target_inst)
    if t not in sel:
        sel.append(t)
    return sel


def case_logits(case):
    """(B, O) float32 logits whose values are all bfloat16 numbers (so both dtypes rank alike): normal draws; even rows
    favour the item's slot; row 0 also has the same maximum again in the LAST slot (a tie: the first wins); row 1 is
    all -inf (arg-max 0); row 2 has NaN in slots 3 and 5 (NaN is the greatest: 3)."""
    import torch
    name, O, mode, seed, items = case
    x = np.random.default_rng(seed).standard_normal((len(items), O)).astype(np.float32)
    for r, it in enumerate(items):
        if r % 2 == 0:
            x[r, it[2]] = 8.0
    x[0, O - 1] = 8.0
    x[1, :] = -np.inf
    x[2, 3] = x[2, 5] = np.nan
    return torch.from_numpy(x).to(torch.bfloat16).float()


# ---- the float64 restatement ---------------------------------------------------------------------------------------
def box_of(points):
    """convert_pc_to_box on the loader's float64 rows: min / max of float32 values, centre and size in float64."""
    p = np.asarray(points, dtype=np.float64)
    lo, hi = p.min(0), p.max(0)
    return np.concatenate([(lo + hi) / 2, hi - lo])


def iou(b1, b2):
    """box3d_iou on construct_bbox_corners' corners, in the reference's order of operations, float64."""
    lo1, hi1 = b1[:3] + (-(b1[3:] / 2)), b1[:3] + b1[3:] / 2
    lo2, hi2 = b2[:3] + (-(b2[3:] / 2)), b2[:3] + b2[3:] / 2
    a, b = np.maximum(lo1, lo2), np.minimum(hi1, hi2)
    d = np.maximum(b - a, 0)
    inter = d[0] * d[1] * d[2]
    v1 = (hi1[0] - lo1[0]) * (hi1[1] - lo1[1]) * (hi1[2] - lo1[2])
    v2 = (hi2[0] - lo2[0]) * (hi2[1] - lo2[1]) * (hi2[2] - lo2[2])
    return inter / (v1 + v2 - inter + 1e-8)


def scene_boxes(s):
    """(boxes of the kept annotated objects, boxes of the non-empty proposals, their labels)."""
    ids, _ = kept(s)
    gt = [box_of(s["points"][s["instance_labels"] == i]) for i in ids]
    keep = [q for q in range(len(s["masks"])) if s["masks"][q].any()]
    prop = [box_of(s["points"][s["masks"][q] == 1]) for q in keep]
    return gt, prop, [s["prop_labels"][q] for q in keep]


def restate_item(s, target_inst, mode, O):
    """-> iou25 (O,), iou50 (O,), tgt_id, labels (O,) as the wrapper pads them."""
    ids, labels = kept(s)
    gt, prop, prop_labels = scene_boxes(s)
    f25, f50, lab = np.zeros(O, np.int64), np.zeros(O, np.int64), np.full(O, -100, np.int64)
    t = ids.index(target_inst)
    if mode == "gt":
        sel = gt_selection(s, target_inst)
        slot = sel.index(t)
        f25[slot] = f50[slot] = 1
        lab[:len(sel)] = [labels[i] for i in sel]
        return f25, f50, slot, lab
    tgt = len(prop)
    for i, b in enumerate(prop):
        v = iou(b, gt[t])
        if v >= 0.25:
            f25[i] = 1
            tgt = i
        if v >= 0.5:
            f50[i] = 1
        lab[i] = prop_labels[i]
        for j, g in enumerate(gt):
            if iou(g, b) >= 0.25:
                lab[i] = labels[j]
                break
    return f25, f50, tgt, lab


def restate_case(case):
    name, O, mode, seed, items = case
    r = [restate_item(scene(sc), inst, mode, O) for sc, inst, _ in items]
    return (np.stack([x[0] for x in r]), np.stack([x[1] for x in r]), np.asarray([x[2] for x in r], np.int64),
            np.stack([x[3] for x in r]))


def pack(scenes=SCENE_NAMES, device="cpu", records=True):
    """The scenes as one PackedScans (annotated objects with their labels, then the proposals), finalized."""
    from sceneverse_amd.data import gpu_objects as G
    packed = G.PackedScans(device, records=records)
    for n in scenes:
        s = scene(n)
        packed.add_scan(n, s["points"], s["colors"], s["instance_labels"], s["inst_ids"], inst_labels=s["inst_labels"])
        packed.add_proposals(n, s["points"], s["colors"], s["masks"], s["prop_labels"])
    return packed.finalize()


def case_inputs(packed, case):
    """-> row_obj (B,O) int32 host table, tgt_obj (scene-local positions), scan ids."""
    from sceneverse_amd.data import gpu_objects as G
    name, O, mode, seed, items = case
    sids = [it[0] for it in items]
    tgt = [kept(scene(sc))[0].index(inst) for sc, inst, _ in items]
    if mode == "gt":
        rows = G.batch_rows(packed, sids, O, obj_select=[gt_selection(scene(sc), inst) for sc, inst, _ in items])
    else:
        rows = G.batch_rows(packed, sids, O, proposals=True)
    return rows, tgt, sids
