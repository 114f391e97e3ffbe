"""The augmented object path on the host: the restatement of tests/objaug_cases.py against the reference's own
outputs (tests/golden/obj_aug_ref.npz, written by tests/golden/make_golden_objaug.py), and the laws of
`draw_aug_params` (sceneverse_amd/data/gpu_objects.py) against DataAugmentor.scene_aug / obj_aug
(data/datasets/data_augmentor.py:39-154).  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import obj_processing as O  # noqa: E402
import objaug_cases as C  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "obj_aug_ref.npz"))
IDS = [c[0] for c in C.CASES]


def _ref(name):
    return GOLD[f"{name}/fts"], GOLD[f"{name}/locs"], GOLD[f"{name}/boxes"]


@pytest.mark.parametrize("mode", ["f32", "f64"])
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_restatement_reproduces_reference_within_noise(case, mode):
    """`noise` is max |reference - float64 restatement| per object and quantity: the float64 mode meets it by
    construction, the mode with the reference's float32 rounding points has to stay inside it as well (it is in
    fact bit-equal where the tensor library is the one the fixture was written with)."""
    name = case[0]
    d = C.unpack_draws(GOLD, name)
    got = C.restate(O.to_obj_pcds(C.case_objs(case)), d, mode)
    for q, e in C.errors(got, _ref(name)).items():
        assert np.all(e <= GOLD[f"{name}/noise_{q}"]), (q, e, GOLD[f"{name}/noise_{q}"])
    # the sizes are taken in float64 before the tensor conversion: bit-equal to float32(float64 value) in either mode
    assert np.array_equal(got[1][:, 3:], GOLD[f"{name}/locs"][:, 3:])
    assert np.array_equal(got[2][:, 3:], GOLD[f"{name}/boxes"][:, 3:])


def test_fixture_covers_the_knobs_it_claims():
    d = C.unpack_draws(GOLD, "pub_train")
    assert d["scene_rot"] is not None
    assert all(d[k] is None for k in ("scene_flip", "scene_scale", "scene_trans", "rgb_delta", "obj_jitter", "obj_trans",
                                      "obj_rot", "noise", "perm"))
    d = C.unpack_draws(GOLD, "pub_val")
    assert all(d[k] is None for k in C.AUG_KEYS + ("obj_trans", "obj_rot", "noise", "perm"))
    for name in ("all_train", "all_p300"):
        d = C.unpack_draws(GOLD, name)
        assert all(d[k] is not None for k in C.AUG_KEYS + ("obj_trans", "obj_rot", "noise", "perm"))
        assert not np.array_equal(d["scene_flip"], np.eye(3))
    assert GOLD["all_p300/idx"].shape == (4, 300)


def _z_rotations():
    out = []
    for t in (0.0, math.pi / 2, math.pi, math.pi * 3 / 2):
        out.append(np.array([[math.cos(t), math.sin(t), 0], [-math.sin(t), math.cos(t), 0], [0, 0, 1]]))
    return out


def test_published_config_draws_z_rotations_only():
    a = G.draw_aug_params(C.PUBLISHED, "train", 64, 80, np.random.default_rng(0))
    zs = _z_rotations()
    seen = set()
    for r in a.scene_rot:
        hit = [i for i, z in enumerate(zs) if np.array_equal(r, z)]
        assert len(hit) == 1
        seen.add(hit[0])
    assert seen == {0, 1, 2, 3}
    for name in ("scene_flip", "scene_scale", "scene_trans", "rgb_delta"):
        assert all(v is None for v in getattr(a, name))
    # aug_list names scene_aug only: the obj_aug block (its pts_shuffle included) is never read
    assert a.obj_trans is None and a.obj_rot is None and a.obj_jitter is None and a.pts_shuffle is None
    tab, row_aug = a.table(64, 80)
    assert tab.shape == (64, G.AUG_STRIDE) and np.all(tab[:, 0] == G.AUG_SCENE_ROT)
    assert np.array_equal(row_aug.reshape(64, 80), np.repeat(np.arange(64)[:, None], 80, 1))
    assert np.array_equal(tab[:, 23:32].reshape(64, 3, 3), np.stack(a.scene_rot, 0))


@pytest.mark.parametrize("cfg", [C.PUBLISHED, C.ALL_KNOBS], ids=["published", "all"])
def test_other_splits_draw_nothing(cfg):
    for split in ("val", "test"):
        a = G.draw_aug_params(cfg, split, 4, 5, np.random.default_rng(1))
        assert all(getattr(a, f) is None for f in a.__dataclass_fields__)
        tab, row_aug = a.table(4, 5)
        assert tab.shape == (0, G.AUG_STRIDE) and np.all(row_aug == -1)
    assert G.draw_aug_params(None, "train", 4, 5, np.random.default_rng(1)).table(4, 5)[0].shape[0] == 0


def test_all_knobs_laws():
    B, O_ = 400, 3
    a = G.draw_aug_params(C.ALL_KNOBS, "train", B, O_, np.random.default_rng(2))
    # flips: exactly the four matrices of data_augmentor.py:54-66, the no-op among them
    flips = [np.diag(v) for v in ([-1.0, 1, 1], [1.0, -1, 1], [-1.0, -1, 1], [1.0, 1, 1])]
    seen = set()
    for m in a.scene_flip:
        hit = [i for i, f in enumerate(flips) if np.array_equal(m, f)]
        assert len(hit) == 1
        seen.add(hit[0])
    assert seen == {0, 1, 2, 3}
    s = np.array(a.scene_scale)
    assert s.min() >= 0.9 and s.max() < 1.1 and s.max() - s.min() > 0.15
    # rotations are proper and bounded by `value`: |theta_z| <= 0.1 * pi for the objects (x and y have value 0)
    for r in a.scene_rot:
        assert np.allclose(r @ r.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(r) - 1) < 1e-12
    for b in range(B):
        for o in range(O_):
            r = a.obj_rot[b][o]
            assert np.array_equal(r[2], [0, 0, 1]) and np.array_equal(r[:, 2], [0, 0, 1])
            th = math.atan2(r[0, 1], r[0, 0])             # the reference's rz = [[c, s, 0], [-s, c, 0], [0, 0, 1]]
            assert abs(th) <= 0.1 * math.pi + 1e-12
    t = np.array(a.scene_trans)
    assert abs(t.mean()) < 6 / math.sqrt(t.size) and abs(t.std() - 1) < 0.1
    ot = np.array(a.obj_trans)
    assert ot.shape == (B, O_, 3) and abs(ot.std() - 0.1) < 0.01
    rgb = np.array(a.rgb_delta)
    assert abs(rgb.std() - 0.1) < 0.01
    assert a.obj_jitter == [0.01] * B and a.pts_shuffle == [True] * B
    tab, row_aug = a.table(B, O_)
    assert tab.shape == (B * O_, G.AUG_STRIDE) and np.all(tab[:, 0] == 255)
    assert np.array_equal(row_aug, np.arange(B * O_))
    assert np.array_equal(tab[4, 2:5], [0.01] * 3) and np.array_equal(tab[4, 8:11], a.obj_trans[1][1])
    assert np.array_equal(tab[4, 32:41].reshape(3, 3), a.obj_rot[1][1]) and tab[4, 1] == a.scene_scale[1]


def _with(cfg, aug, knob, **kw):
    import copy
    c = copy.deepcopy(cfg)
    c[aug][knob].update(kw)
    return c


@pytest.mark.parametrize("aug,knob,field", [("scene_aug", "translation", "scene_trans"), ("scene_aug", "scaling", "scene_scale"),
                                            ("scene_aug", "flip", "scene_flip"), ("scene_aug", "rotation", "scene_rot"),
                                            ("obj_aug", "translation", "obj_trans"), ("obj_aug", "rotation", "obj_rot")])
def test_p_and_enabled(aug, knob, field):
    def fired(cfg):
        a = G.draw_aug_params(cfg, "train", 50, 2, np.random.default_rng(3))
        v = getattr(a, field)
        flat = v if aug == "scene_aug" else [x for per in v for x in per]
        return sum(x is not None for x in flat), len(flat)
    n, tot = fired(_with(C.ALL_KNOBS, aug, knob, p=0.0))
    assert n == 0
    n, tot = fired(_with(C.ALL_KNOBS, aug, knob, p=1.0))
    assert n == tot
    n, tot = fired(_with(C.ALL_KNOBS, aug, knob, p=0.5))
    assert 0 < n < tot
    n, tot = fired(_with(C.ALL_KNOBS, aug, knob, enabled=False))
    assert n == 0


def test_axis_aligned_rotation_forms_and_shuffle():
    """rx, ry, rz as data_augmentor.py:78-89 writes them, multiplied in a shuffled order when `shuffle` is set."""
    cfg = _with(C.ALL_KNOBS, "scene_aug", "rotation", axis_align=True, value=[1.0, 0.0, 0.0], shuffle=False)
    a = G.draw_aug_params(cfg, "train", 40, 1, np.random.default_rng(4))
    want = [np.array([[1, 0, 0], [0, math.cos(t), -math.sin(t)], [0, math.sin(t), math.cos(t)]])
            for t in (0.0, math.pi / 2, math.pi, math.pi * 3 / 2)]
    assert all(any(np.array_equal(r, w) for w in want) for r in a.scene_rot)
    cfg = _with(C.ALL_KNOBS, "scene_aug", "rotation", axis_align=True, value=[0.0, 1.0, 0.0], shuffle=False)
    a = G.draw_aug_params(cfg, "train", 40, 1, np.random.default_rng(4))
    want = [np.array([[math.cos(t), 0, math.sin(t)], [0, 1, 0], [-math.sin(t), 0, math.cos(t)]])
            for t in (0.0, math.pi / 2, math.pi, math.pi * 3 / 2)]
    assert all(any(np.array_equal(r, w) for w in want) for r in a.scene_rot)
    # x and z quarter turns do not commute: with shuffle both orders of the product turn up
    cfg = _with(C.ALL_KNOBS, "scene_aug", "rotation", axis_align=True, value=[1.0, 0.0, 1.0], shuffle=True)
    a = G.draw_aug_params(cfg, "train", 400, 1, np.random.default_rng(5))
    cfg["scene_aug"]["rotation"]["shuffle"] = False
    b = G.draw_aug_params(cfg, "train", 400, 1, np.random.default_rng(5))
    key = lambda rs: {tuple(np.rint(r).astype(int).reshape(-1)) for r in rs}
    assert len(key(a.scene_rot)) > len(key(b.scene_rot))


def test_missing_augmentor_block_and_unknown_name():
    cfg = {"aug_list": ["scene_aug", "obj_aug"], "scene_aug": C.PUBLISHED["scene_aug"]}   # obj_aug listed, not defined
    a = G.draw_aug_params(cfg, "train", 3, 2, np.random.default_rng(6))
    assert a.obj_trans is None and all(r is not None for r in a.scene_rot)
    with pytest.raises(ValueError):
        G.draw_aug_params({"aug_list": ["bg_aug"], "bg_aug": {}}, "train", 1, 1, np.random.default_rng(0))
