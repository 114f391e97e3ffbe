"""TEST INFRASTRUCTURE -- the laws of gps_aug_draw (both modes) and gps_item_rows of include/gps_hip.h, restated in
numpy / `math` (the "mirror"), and the configs the tests of the device-drawn loader share.

What is restated: per output row (b, o) of a (B, O) batch either "nothing" (row_aug = -1) or the 48-double entry of the
parameter table gps_obj_processing_aug reads; per scene the build_rotate_mat index and its float32 matrix; per row of
item ids the look-ups of gps_item_rows.  Every draw is a word of the counter stream rng_u32 of csrc/gps_dropout.h; the
few lines that emulate it are those of tests/test_dropout_hash.py (mix32, seed_fold).

Where the law is integer (which knob fires, flip, angle index, permutation) or a fixed sequence of IEEE operations
(scale, the axis-aligned table and its products) the mirror is exact.  The free angles, translations and colour
deltas pass through sin / cos / log / sqrt / cospi: here through `math`, on the device through its own libm --
tests/test_gpu_augdraw.py states the tolerance between the two.
"""
from __future__ import annotations

import copy
import math

import numpy as np

from objaug_cases import ALL_KNOBS, PUBLISHED

M32 = np.uint64(0xFFFFFFFF)
M64 = (1 << 64) - 1
STRIDE = 48
FLIP, SCALE, SCENE_TRANS, SCENE_ROT, RGB, OBJ_TRANS, OBJ_ROT, JITTER = 1, 2, 4, 8, 16, 32, 64, 128
# the counters of include/gps_hip.h (GPS_AUG_K_*)
K_TRANS_P, K_TRANS, K_SCALE_P, K_SCALE, K_FLIP_P, K_FLIP, K_ROT_P, K_ROT_ANGLE, K_ROT_PERM, K_RGB = 0, 1, 7, 8, 9, 10, 11, 12, 15, 16
ANGLES = (0.0, math.pi / 2, math.pi, math.pi * 3 / 2)
COS4 = tuple(math.cos(a) for a in ANGLES)
SIN4 = tuple(math.sin(a) for a in ANGLES)
PERM6 = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


# ---- the counter stream (csrc/gps_dropout.h), as tests/test_dropout_hash.py emulates it --------------------------------
def mix32(x):
    x = x.astype(np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x21F0AAAD)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x735A2D97)) & M32
    x ^= x >> np.uint64(15)
    return x


def seed_fold(seed):
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    return mix32(np.array([lo], dtype=np.uint64) ^ mix32(np.array([(hi + np.uint64(0x9E3779B9)) & M32], dtype=np.uint64)))[0]


def rng_u32(seed, idx):
    """rng_u32(seed, idx) for a 64-bit seed and an array (or one) 64-bit index -> uint64 array of 32-bit words."""
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    folded = ((idx & M32) + ((idx >> np.uint64(32)) * np.uint64(0x85EBCA6B) & M32)) & M32
    return mix32(folded ^ seed_fold(int(seed) & M64))


# ---- the configs --------------------------------------------------------------------------------------------------------
def _variant(p=None, axis_align=None, scene_value=None, obj_value=None):
    cfg = copy.deepcopy(ALL_KNOBS)
    for aug in ("scene_aug", "obj_aug"):
        for knob in cfg[aug].values():
            if isinstance(knob, dict) and "p" in knob and p is not None:
                knob["p"] = p
        if axis_align is not None:
            cfg[aug]["rotation"]["axis_align"] = axis_align
    if scene_value is not None:
        cfg["scene_aug"]["rotation"]["value"] = scene_value
    if obj_value is not None:
        cfg["obj_aug"]["rotation"]["value"] = obj_value
    return cfg


# every p = 0.5 and axis-aligned rotations; `value` as in ALL_KNOBS (0.1 * angle goes through sin / cos) ...
HALF_AXIS = _variant(p=0.5, axis_align=True)
# ... and with values 0 / 1 only, where every rotation comes from the constant table and must be EQUAL
HALF_AXIS_TABLE = _variant(p=0.5, axis_align=True, scene_value=[1.0, 1.0, 1.0], obj_value=[0.0, 1.0, 1.0])
# the published config with its rotation at p = 0.5: scenes for which nothing fires (row_aug = -1)
PUBLISHED_HALF = copy.deepcopy(PUBLISHED)
PUBLISHED_HALF["scene_aug"]["rotation"]["p"] = 0.5
CONFIGS = {"published": PUBLISHED, "all": ALL_KNOBS, "half_axis": HALF_AXIS, "half_axis_table": HALF_AXIS_TABLE,
           "published_half": PUBLISHED_HALF}


def check_key(key):
    if key is None:
        return False
    if isinstance(key, bool):
        return key
    if isinstance(key, dict):
        return bool(key.get("enabled", True))
    return True


def knob_p(key):
    return float(key["p"]) if isinstance(key, dict) and "p" in key else 1.0


def per_object(cfg):
    """Some per-object knob is on: the table has B * O entries (else B)."""
    if "obj_aug" not in cfg["aug_list"] or "obj_aug" not in cfg:
        return False
    return check_key(cfg["obj_aug"].get("translation")) or check_key(cfg["obj_aug"].get("rotation"))


def table_rotations(cfg):
    """{'scene': bool, 'obj': bool}: that rotation, when it fires, is built from the constant table alone (axis-aligned,
    every value 0 or 1) -- the entries that must be EQUAL on the device."""
    out = {}
    for name, aug in (("scene", "scene_aug"), ("obj", "obj_aug")):
        r = cfg.get(aug, {}).get("rotation") if aug in cfg["aug_list"] else None
        out[name] = bool(r and isinstance(r, dict) and r.get("axis_align") and all(v in (0.0, 1.0) for v in r["value"]))
    return out


# ---- the law -------------------------------------------------------------------------------------------------------------
class Stream:
    def __init__(self, seed, b, O, slot):
        self.seed = (int(seed) + 6) & M64
        self.base = (b * (O + 1) + slot) * 64

    def u32(self, k):
        return int(rng_u32(self.seed, self.base + k)[0])

    def fires(self, k, p):
        return self.u32(k) < int(p * 4294967296.0)

    def choice(self, k, n):
        return (self.u32(k) * n) >> 32

    def uniform(self, k):
        return self.u32(k) * 2.0 ** -32

    def normal(self, k):
        u1, u2 = (self.u32(k) + 1.0) * 2.0 ** -32, self.u32(k + 1) * 2.0 ** -32
        return math.sqrt(-2.0 * math.log(u1)) * cospi(2.0 * u2)


def cospi(x):
    """cos(pi x) for a dyadic x in [0, 2) with the argument reduced exactly: |pi r| <= pi / 4 reaches cos / sin, whose
    relative error is then that of the rounded product pi r (a plain math.cos(pi * x) loses the digits near the zeros)."""
    q = math.floor(2.0 * x + 0.5)                # the nearest multiple of 1/2
    r = x - q * 0.5                              # exact; |r| <= 1/4
    q = int(q) & 3
    if q == 0:
        return math.cos(math.pi * r)
    if q == 1:
        return -math.sin(math.pi * r)
    if q == 2:
        return -math.cos(math.pi * r)
    return math.sin(math.pi * r)


def mat3_mul(a, b):
    return [[(a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j] for j in range(3)] for i in range(3)]


def draw_rotation(st, cfg):
    c, s = [0.0] * 3, [0.0] * 3
    for i in range(3):
        v = float(cfg["value"][i])
        if cfg["axis_align"]:
            a = st.choice(K_ROT_ANGLE + i, 4)
            if v == 0.0:
                c[i], s[i] = COS4[0], SIN4[0]
            elif v == 1.0:
                c[i], s[i] = COS4[a], SIN4[a]
            else:
                th = ANGLES[a] * v
                c[i], s[i] = math.cos(th), math.sin(th)
        else:
            th = (st.uniform(K_ROT_ANGLE + i) * 2.0 * math.pi - math.pi) * v
            c[i], s[i] = math.cos(th), math.sin(th)
    m = [[[1.0, 0.0, 0.0], [0.0, c[0], -s[0]], [0.0, s[0], c[0]]],
         [[c[1], 0.0, s[1]], [0.0, 1.0, 0.0], [-s[1], 0.0, c[1]]],
         [[c[2], s[2], 0.0], [-s[2], c[2], 0.0], [0.0, 0.0, 1.0]]]
    perm = PERM6[st.choice(K_ROT_PERM, 6)] if cfg.get("shuffle", False) else PERM6[0]
    return np.array(mat3_mul(mat3_mul(m[perm[0]], m[perm[1]]), m[perm[2]]), dtype=np.float64)


def draw_translation(st, cfg):
    return np.array([st.normal(K_TRANS + 2 * i) * float(cfg["value"][i]) for i in range(3)], dtype=np.float64)


def mirror_entry(cfg, B, O, seed, b, o):
    """The entry of output row (b, o): (flags, 48 doubles); flags == 0 is "nothing" (row_aug = -1)."""
    e, flags = np.zeros(STRIDE, dtype=np.float64), 0
    on = [n for n in cfg["aug_list"] if n in cfg]
    if "scene_aug" in on:
        c, st = cfg["scene_aug"], Stream(seed, b, O, 0)
        k = c.get("translation")
        if check_key(k) and st.fires(K_TRANS_P, knob_p(k)):
            e[5:8] = draw_translation(st, k)
            flags |= SCENE_TRANS
        k = c.get("scaling")
        if check_key(k) and st.fires(K_SCALE_P, knob_p(k)):
            e[1] = st.uniform(K_SCALE) * (float(k["value"][1]) - float(k["value"][0])) + float(k["value"][0])
            flags |= SCALE
        k = c.get("flip")
        if check_key(k) and st.fires(K_FLIP_P, knob_p(k)):
            kind = st.choice(K_FLIP, 4)
            e[14:23] = np.diag([-1.0 if kind in (0, 2) else 1.0, -1.0 if kind in (1, 2) else 1.0, 1.0]).reshape(-1)
            flags |= FLIP
        k = c.get("rotation")
        if check_key(k) and st.fires(K_ROT_P, knob_p(k)):
            e[23:32] = draw_rotation(st, k).reshape(-1)
            flags |= SCENE_ROT
        if check_key(c.get("color_jitter")):
            e[11:14] = [st.normal(K_RGB + 2 * i) * 0.1 for i in range(3)]
            flags |= RGB
    if "obj_aug" in on:
        c, st = cfg["obj_aug"], Stream(seed, b, O, 1 + o)
        k = c.get("translation")
        if check_key(k) and st.fires(K_TRANS_P, knob_p(k)):
            e[8:11] = draw_translation(st, k)
            flags |= OBJ_TRANS
        k = c.get("rotation")
        if check_key(k) and st.fires(K_ROT_P, knob_p(k)):
            e[32:41] = draw_rotation(st, k).reshape(-1)
            flags |= OBJ_ROT
        if check_key(c.get("random_jitter")):
            e[2:5] = np.broadcast_to(np.asarray(c["random_jitter"]["value"], dtype=np.float64).reshape(-1), (3,))
            flags |= JITTER
    e[0] = flags
    return flags, e


def mirror_rows(cfg, split, B, O, seed):
    """-> (B * O) list, per output row None ("nothing") or its 48-double entry; None altogether off the train split."""
    if cfg is None or split != "train":
        return None
    rows = []
    for b in range(B):
        for o in range(O if per_object(cfg) else 1):
            flags, e = mirror_entry(cfg, B, O, seed, b, o)
            rows.append(e if flags else None)
        if not per_object(cfg):
            rows.extend([rows[-1]] * (O - 1))
    return rows


def mirror_table(cfg, split, B, O, seed):
    """The mirror in the layout the device writes: (entries (n_aug, 48), row_aug (B * O,) int32), a silent entry zeros."""
    per = per_object(cfg)
    n = B * O if per else B
    entries, row_aug = np.zeros((n, STRIDE), dtype=np.float64), np.full(B * O, -1, dtype=np.int32)
    for r, e in enumerate(mirror_rows(cfg, split, B, O, seed)):
        if e is not None:
            at = r if per else r // O
            entries[at], row_aug[r] = e, at
    return entries, row_aug


def resolve(entries, row_aug):
    """A device (or mirror) table resolved per output row: None where row_aug is -1, else the row's entry."""
    return [None if a < 0 else np.asarray(entries[a]) for a in np.asarray(row_aug).tolist()]


def mirror_rot(split, rot_aug, B, O, seed):
    """build_rotate_mat by the law: (idx (B,), mats (B, 3, 3) float32, row_rot (B * O,) int32); None off the train split."""
    if split != "train" or not rot_aug:
        return None
    idx = ((rng_u32((int(seed) + 7) & M64, np.arange(B, dtype=np.uint64)) * np.uint64(4)) >> np.uint64(32)).astype(np.int64)
    mats = np.zeros((B, 3, 3), dtype=np.float32)
    for b, a in enumerate(idx.tolist()):
        mats[b] = np.array([[COS4[a], -SIN4[a], 0], [SIN4[a], COS4[a], 0], [0, 0, 1]], dtype=np.float32)
    row_rot = np.repeat(np.where(idx == 0, -1, np.arange(B)), O).astype(np.int32)
    return idx, mats, row_rot


# ---- gps_item_rows ---------------------------------------------------------------------------------------------------------
def restate_item_rows(table, item_ids, pick=None, seed=0):
    """table: dict(item_scan, item_tgt, item_label, item_sent (n_items,); scan_range, prop_range (n_scans, 2);
    caps: per scan a list of text ids; default_caption).  -> dict of int32 arrays under gps_item_rows' output names."""
    B = len(item_ids)
    out = {k: np.zeros((B, 2), np.int32) for k in ("scan_range", "prop_range")}
    out.update({k: np.zeros(B, np.int32) for k in ("tgt_obj", "tgt_label", "sent_idx", "cap_idx", "scan_idx")})
    n_items, n_scans = len(table["item_scan"]), len(table["scan_range"])
    for b, i in enumerate(item_ids):
        s = int(table["item_scan"][i]) if 0 <= i < n_items else -1
        if not 0 <= s < n_scans:
            out["sent_idx"][b] = out["cap_idx"][b] = out["scan_idx"][b] = -1
            continue
        out["scan_range"][b], out["prop_range"][b] = table["scan_range"][s], table["prop_range"][s]
        out["tgt_obj"][b], out["tgt_label"][b] = table["item_tgt"][i], table["item_label"][i]
        out["sent_idx"][b], out["scan_idx"][b] = table["item_sent"][i], s
        caps = table["caps"][s]
        if not caps:
            out["cap_idx"][b] = table["default_caption"]
            continue
        if pick is not None:
            p = int(pick[b]) if 0 <= int(pick[b]) < len(caps) else 0
        else:
            p = int(rng_u32((int(seed) + 5) & M64, b)[0]) % len(caps)
        out["cap_idx"][b] = caps[p]
    return out
