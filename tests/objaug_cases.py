"""TEST INFRASTRUCTURE -- the cases of the augmented object path and a restatement of it with the draws passed in.

What is restated: DataAugmentor.update_data_dict (data/datasets/data_augmentor.py:156-215) followed by
ScanBase._obj_processing_aug (data/datasets/base.py:742-776), for the objects of one scene:

    flip -> scale about the mean of ALL points -> subsample -> jitter (z - 0.5) * scale -> size = max - min
    -> scene translation -> object translation -> scene rotation x @ R -> object rotation about the sample mean
    -> colour delta -> point shuffle -> centre, box, x -= centre, x /= max(max ||x||, 1e-6)

Two rounding modes:
    "f64"  everything in float64, rounded to float32 once at the end (the sizes from their float64 value).  This is
           the target the device kernel is written against.
    "f32"  the reference's own rounding points: with a scene rotation the whole scene becomes a float32 tensor right
           before it (data_augmentor.py:194) and every later step stores float32 (its matrix products and sums with
           the float64 parameters still run in float64 on the float32 values); without one the float64 arrays reach
           base.py:750 and are rounded there.  base.py:753-769 then runs in float32, restated with the same tensor
           operations.

Shared by tests/golden/make_golden_objaug.py (which runs the reference itself and stores its outputs, the captured
draws and `noise` = max |reference - "f64" restatement| per object and quantity), tests/test_objects_aug_host.py and
tests/test_gpu_objects_aug.py.
"""
from __future__ import annotations

import numpy as np

# the object-size list of the case u8_train of tests/golden/make_golden_objproc.py
KS = [1, 7, 255, 256, 257, 900, 3000, 40, 512, 1500]

# The `data_aug:` block every YAML under configs/final/ of the reference carries.  aug_list names scene_aug only, so
# the obj_aug block -- its `pts_shuffle: True` included -- never runs: a published training scene gets one of the four
# z-rotations and nothing else.
PUBLISHED = {
    "aug_list": ["scene_aug"],
    "scene_aug": {
        "translation": {"enabled": False, "value": [1.0, 1.0, 1.0], "p": 1.0},
        "scaling": {"enabled": False, "p": 1.0, "value": [0.9, 1.1]},
        "flip": {"enabled": False, "p": 0.5},
        "rotation": {"enabled": True, "p": 1.0, "axis_align": True, "value": [0.0, 0.0, 1.0], "shuffle": True},
        "color_jitter": False,
        "order_shuffle": False,
    },
    "obj_aug": {
        "translation": {"enabled": False, "value": [0.1, 0.1, 0.1], "p": 1.0},
        "rotation": {"enabled": False, "p": 1.0, "axis_align": False, "value": [0.0, 0.0, 0.1], "shuffle": True},
        "random_jitter": {"enabled": False, "value": 0.01, "accord_to_size": False, "p": 1.0},
        "pts_shuffle": True,
    },
}

# every knob on (the same schema and magnitudes, both augmentors listed, free angles about all three axes)
ALL_KNOBS = {
    "aug_list": ["scene_aug", "obj_aug"],
    "scene_aug": {
        "translation": {"enabled": True, "value": [1.0, 1.0, 1.0], "p": 1.0},
        "scaling": {"enabled": True, "p": 1.0, "value": [0.9, 1.1]},
        "flip": {"enabled": True, "p": 1.0},
        "rotation": {"enabled": True, "p": 1.0, "axis_align": False, "value": [0.1, 0.1, 1.0], "shuffle": True},
        "color_jitter": True,
        "order_shuffle": True,
    },
    "obj_aug": {
        "translation": {"enabled": True, "value": [0.1, 0.1, 0.1], "p": 1.0},
        "rotation": {"enabled": True, "p": 1.0, "axis_align": False, "value": [0.0, 0.0, 0.1], "shuffle": True},
        "random_jitter": {"enabled": True, "value": 0.01, "accord_to_size": False, "p": 1.0},
        "pts_shuffle": True,
    },
}
CONFIGS = {"published": PUBLISHED, "all": ALL_KNOBS}

# (name, scene seed, numpy global seed, num_points, config, split, object sizes)
CASES = [
    ("pub_train", 11, 201, 256, "published", "train", KS),
    ("all_train", 11, 202, 256, "all", "train", KS),
    ("pub_val", 11, 203, 256, "published", "val", KS),
    # the second register slot is partly filled (300 = 256 + 44); scaling walks a 3000-point object: two trips of the
    # 4-wide stream loop and a tail
    ("all_p300", 15, 204, 300, "all", "train", [3000, 120, 300, 299]),
]
QUANTITIES = ("xyz", "rgb", "locs", "boxes")


def case_objs(case):
    """The raw objects of a case, (points f32 (k,3), colours u8 (k,3)) each, regenerated from its seed."""
    from oracle import obj_processing as O
    name, scene_seed, np_seed, num_points, cfg, split, ks = case
    return O.synth_scene(np.random.default_rng(scene_seed), len(ks), np.uint8, ks)


AUG_KEYS = ("scene_flip", "scene_scale", "scene_trans", "scene_rot", "rgb_delta", "obj_jitter")


def pack_draws(prefix, n, aug_dict, idx, noise, perm):
    """The captured draws of one scene as flat arrays (absent knobs are simply missing keys)."""
    out = {f"{prefix}/idx": np.stack(idx, 0).astype(np.int32)}
    for k in AUG_KEYS:
        if aug_dict.get(k) is not None:
            out[f"{prefix}/{k}"] = np.asarray(aug_dict[k], dtype=np.float64)
    for k, shape in (("obj_trans", (3,)), ("obj_rot", (3, 3))):
        v = aug_dict.get(k)
        if v and any(x is not None for x in v):
            out[f"{prefix}/{k}"] = np.stack([np.zeros(shape) if x is None else np.asarray(x, np.float64) for x in v], 0)
            out[f"{prefix}/{k}_on"] = np.array([x is not None for x in v])
    if noise:
        out[f"{prefix}/noise"] = np.stack(noise, 0)
    if perm:
        out[f"{prefix}/perm"] = np.stack(perm, 0).astype(np.int32)
    return out


def unpack_draws(gold, prefix):
    """-> dict: idx (n,P), noise (n,P,3) | None, perm (n,P) | None, the scene knobs (array | None), obj_trans / obj_rot
    (list with None for an object left alone | None)."""
    d = {"idx": gold[f"{prefix}/idx"]}
    n = d["idx"].shape[0]
    for k in AUG_KEYS + ("noise", "perm"):
        d[k] = gold[f"{prefix}/{k}"] if f"{prefix}/{k}" in gold else None
    for k in ("obj_trans", "obj_rot"):
        if f"{prefix}/{k}" in gold:
            on = gold[f"{prefix}/{k}_on"]
            d[k] = [gold[f"{prefix}/{k}"][i] if on[i] else None for i in range(n)]
        else:
            d[k] = None
    return d


def replay_order(d):
    """(idx, noise) in the order the point shuffle left the rows: what a replay hands to the device."""
    idx, noise = d["idx"], d["noise"]
    if d["perm"] is not None:
        idx = np.take_along_axis(idx, d["perm"], 1)
        if noise is not None:
            noise = np.take_along_axis(noise, d["perm"][:, :, None], 1)
    return idx, noise


def restate(obj_pcds, d, mode="f64"):
    """obj_pcds: list of (k_i, 6) [xyz | rgb / 127.5 - 1]; d: unpack_draws(...).  Returns float32 arrays
    (obj_fts (n,P,6), obj_locs (n,6), obj_boxes (n,6))."""
    assert mode in ("f64", "f32")
    samp, sizes = [], []
    for i, pc in enumerate(obj_pcds):
        pc = np.array(pc, dtype=np.float64)
        if d["scene_flip"] is not None:
            pc[:, :3] = np.matmul(pc[:, :3], d["scene_flip"])
        if d["scene_scale"] is not None:
            c = pc[:, :3].mean(0)
            pc[:, :3] = (pc[:, :3] - c) * d["scene_scale"] + c
        pc = pc[d["idx"][i]]
        if d["obj_jitter"] is not None:
            pc[:, :3] = pc[:, :3] + (d["noise"][i] - 0.5) * d["obj_jitter"]
        sizes.append(pc[:, :3].max(0) - pc[:, :3].min(0))
        if d["scene_trans"] is not None:
            pc[:, :3] += d["scene_trans"]
        if d["obj_trans"] is not None and d["obj_trans"][i] is not None:
            pc[:, :3] += d["obj_trans"][i]
        samp.append(pc)
    size = np.array(sizes).astype(np.float32)
    n = len(samp)
    if mode == "f64":
        P = np.array(samp)
        if d["scene_rot"] is not None:
            P[:, :, :3] = np.matmul(P[:, :, :3], d["scene_rot"])
        for i in range(n):
            if d["obj_rot"] is not None and d["obj_rot"][i] is not None:
                c = P[i][:, :3].mean(0)
                P[i][:, :3] = np.matmul(P[i][:, :3] - c, d["obj_rot"][i]) + c
            if d["rgb_delta"] is not None:
                P[i][:, 3:] += d["rgb_delta"]
            if d["perm"] is not None:
                P[i] = P[i][d["perm"][i]]
        xyz = P[:, :, :3]
        centre = xyz.mean(1)
        box_centre = (xyz.min(1) + xyz.max(1)) / 2
        xyz = xyz - centre[:, None]
        max_dist = np.maximum(np.sqrt((xyz ** 2).sum(2)).max(1), 1e-6)
        P[:, :, :3] = xyz / max_dist[:, None, None]
        return (P.astype(np.float32), np.concatenate([centre.astype(np.float32), size], 1),
                np.concatenate([box_centre.astype(np.float32), size], 1))
    import torch
    if d["scene_rot"] is not None:
        T = torch.Tensor(np.array(samp))                                          # float32 from here on
        T[:, :, :3] = torch.from_numpy(np.matmul(T[:, :, :3].numpy(), d["scene_rot"]))
        for i in range(n):
            if d["obj_rot"] is not None and d["obj_rot"][i] is not None:
                x = T[i][:, :3]
                c = x.mean(0)
                T[i][:, :3] = torch.from_numpy(np.matmul((x - c).numpy(), d["obj_rot"][i]) + c.numpy())
            if d["rgb_delta"] is not None:
                T[i][:, 3:] = torch.from_numpy(T[i][:, 3:].numpy() + d["rgb_delta"])
            if d["perm"] is not None:
                T[i] = T[i][d["perm"][i].astype(np.int64)]
    else:
        for i in range(n):
            if d["obj_rot"] is not None and d["obj_rot"][i] is not None:
                c = samp[i][:, :3].mean(0)
                samp[i][:, :3] = np.matmul(samp[i][:, :3] - c, d["obj_rot"][i]) + c
            if d["rgb_delta"] is not None:
                samp[i][:, 3:] += d["rgb_delta"]
            if d["perm"] is not None:
                samp[i] = samp[i][d["perm"][i]]
        T = torch.Tensor(np.array(samp))
    xyz = T[:, :, :3]
    centre = xyz.mean(1)
    box_centre = (xyz.min(1).values + xyz.max(1).values) / 2
    T[:, :, :3].sub_(T[:, :, :3].mean(1, keepdim=True))
    max_dist = (T[:, :, :3] ** 2).sum(2).sqrt().max(1).values
    max_dist.clamp_(min=1e-6)
    T[:, :, :3].div_(max_dist[:, None, None])
    return (T.numpy(), np.concatenate([centre.numpy(), size], 1), np.concatenate([box_centre.numpy(), size], 1))


def errors(got, ref):
    """max |got - ref| per object for the four quantities, from (fts, locs, boxes) triples -> {quantity: (n,)}."""
    gf, gl, gb = (np.asarray(a, dtype=np.float64) for a in got)
    rf, rl, rb = (np.asarray(a, dtype=np.float64) for a in ref)
    return {"xyz": np.abs(gf[:, :, :3] - rf[:, :, :3]).max((1, 2)), "rgb": np.abs(gf[:, :, 3:] - rf[:, :, 3:]).max((1, 2)),
            "locs": np.abs(gl[:, :3] - rl[:, :3]).max(1), "boxes": np.abs(gb[:, :3] - rb[:, :3]).max(1)}
