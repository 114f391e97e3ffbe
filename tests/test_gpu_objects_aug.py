"""gps_obj_processing_aug (sceneverse_amd/data/gpu_objects.py -> libgps_hip.so) against
  * the reference's own DataAugmentor + ScanBase._obj_processing_aug outputs (tests/golden/obj_aug_ref.npz), replayed
    with the captured draws in both record forms,
  * the float64 restatement of tests/objaug_cases.py for float32-stored colours,
  * properties of the device-drawn mode (sampler, jitter law) and the C ABI's argument checks.

Tolerance of the replays: per object and quantity |got - ref| <= 2 * noise + 1 float32 ulp, where `noise` is the
fixture's max |reference - float64 restatement| (the reference rounds to float32 at the scene rotation or at the tensor
conversion and finishes in float32).  The kernel is written against the float64 restatement, so it sits at 1 * noise
from the reference; the other 1 * noise (+ the final rounding's ulp) is what its own summation order may use.  The
k = 1 object without jitter is no parity target: its centred residue is float32 rounding noise of the REFERENCE
divided by the 1e-6 clamp (0.24 in the fixture); in float64 it is exactly 0."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import obj_processing as O  # noqa: E402
import objaug_cases as C  # noqa: E402
from sceneverse_amd import _native  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402

DEV = "cuda"
GOLD = np.load(os.path.join(HERE, "golden", "obj_aug_ref.npz"))
IDS = [c[0] for c in C.CASES]


def pack(objs, shuffle_seed=0, records=True):
    """Objects -> one raw scan (points interleaved across instances, as on disk) -> PackedScans."""
    pts = np.concatenate([p for p, _ in objs], 0)
    col = np.concatenate([c for _, c in objs], 0)
    lab = np.concatenate([np.full(len(p), 100 + i) for i, (p, _) in enumerate(objs)])
    lab_p = lab[np.argsort(np.random.default_rng(shuffle_seed).random(len(lab)), kind="stable")]
    out_idx = np.empty(len(lab), dtype=np.int64)
    for i in range(len(objs)):
        out_idx[np.flatnonzero(lab_p == 100 + i)] = np.flatnonzero(lab == 100 + i)
    packed = G.PackedScans(DEV, records=records)
    packed.add_scan("s0", pts[out_idx], col[out_idx], lab[out_idx], [100 + i for i in range(len(objs))] + [999])
    return packed.finalize()


def aug_of(d):
    """The captured draws of one scene as a one-scene AugParams."""
    one = lambda v: None if v is None else [v]
    return G.AugParams(scene_flip=one(d["scene_flip"]), scene_scale=one(d["scene_scale"]),
                       scene_trans=one(d["scene_trans"]), scene_rot=one(d["scene_rot"]), rgb_delta=one(d["rgb_delta"]),
                       obj_trans=one(d["obj_trans"]), obj_rot=one(d["obj_rot"]), obj_jitter=one(d["obj_jitter"]),
                       pts_shuffle=one(True if d["perm"] is not None else None))


def replay(packed, d, n, num_points, pad=2, noise_dtype=torch.float64, **kw):
    rows = G.batch_rows(packed, ["s0"], n + pad)
    idx, noise = C.replay_order(d)
    sidx = torch.zeros((1, n + pad, num_points), dtype=torch.int32)
    sidx[0, :n] = torch.from_numpy(idx.astype(np.int32))
    jn = None
    if noise is not None:
        jn = torch.zeros((1, n + pad, num_points, 3), dtype=noise_dtype)
        jn[0, :n] = torch.from_numpy(noise).to(noise_dtype)
    return G.obj_processing_aug(packed, rows, num_points, aug=aug_of(d), sample_idx=sidx, jitter_noise=jn,
                                need_boxes=True, **kw)


def ulp(ref):
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def within(got, ref, noise, what):
    """|got - ref| <= 2 * noise[object] + 1 float32 ulp, elementwise; prints the figure before it asserts."""
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    err = np.abs(got - ref)
    bound = 2 * noise.reshape((-1,) + (1,) * (ref.ndim - 1)) + ulp(ref)
    print(f"{what}: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound), (what, float(err.max()), np.argwhere(err > bound)[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("records", [True, False], ids=["rec16", "two_arrays"])
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_replay_matches_reference(case, records):
    name, scene_seed, np_seed, num_points, cfg, split, ks = case
    objs, n = C.case_objs(case), len(case[6])
    packed = pack(objs, shuffle_seed=scene_seed, records=records)
    assert packed.records == records
    d = C.unpack_draws(GOLD, name)
    out = replay(packed, d, n, num_points)
    fts, locs, boxes = (out[k][0].cpu().numpy() for k in ("obj_fts", "obj_locs", "obj_boxes"))
    ref_f, ref_l, ref_b = GOLD[f"{name}/fts"], GOLD[f"{name}/locs"], GOLD[f"{name}/boxes"]
    assert np.all(np.isfinite(fts)) and np.all(np.isfinite(locs)) and np.all(np.isfinite(boxes))
    parity = np.array([not (k == 1 and d["noise"] is None) for k in ks])
    for o in np.flatnonzero(~parity):             # a single point, no jitter: the centred cloud is exactly the origin
        assert np.all(np.linalg.norm(fts[o, :, :3].astype(np.float64), axis=1) <= 1 + 1e-6)
    within(fts[:n, :, :3][parity], ref_f[:, :, :3][parity], GOLD[f"{name}/noise_xyz"][parity], "xyz")
    within(fts[:n, :, 3:], ref_f[:, :, 3:], GOLD[f"{name}/noise_rgb"], "rgb")
    within(locs[:n, :3], ref_l[:, :3], GOLD[f"{name}/noise_locs"], "locs")
    within(boxes[:n, :3], ref_b[:, :3], GOLD[f"{name}/noise_boxes"], "boxes")
    # sizes: rounded from their float64 value, like the reference's
    for got, ref in ((locs[:n, 3:], ref_l[:, 3:]), (boxes[:n, 3:], ref_b[:, 3:])):
        assert np.all(np.abs(got.astype(np.float64) - ref) <= ulp(ref))
        assert np.mean(got == ref) > 0.999
    # padding slots: dataset_wrapper.py:62-70
    assert np.all(fts[n:] == 1.0) and np.all(locs[n:] == 0.0) and np.all(boxes[n:] == 0.0)
    assert out["obj_masks"][0].tolist() == [True] * n + [False] * 2


@pytest.mark.gpu
def test_f32_colours_and_f32_noise_match_float64_restatement():
    """float32-stored colours (two arrays; the loader scales them in float32) and float32 replay noise, every knob
    on, against the float64 restatement on the same inputs.  Bound: twice the largest `noise` of the fixture's parity
    targets (+ 1 ulp) -- no wider than what any replay above is held to."""
    case = C.CASES[1]
    objs = O.synth_scene(np.random.default_rng(14), len(C.KS), np.float32, C.KS)
    d = dict(C.unpack_draws(GOLD, case[0]))
    d["noise"] = d["noise"].astype(np.float32).astype(np.float64)
    pcds = O.to_obj_pcds(objs)
    assert pcds[0].dtype == np.float32
    want = C.restate(pcds, d, "f64")
    packed = pack(objs, shuffle_seed=3, records=True)
    assert packed.records is False and packed.rgb.dtype == torch.float32
    out = replay(packed, d, len(C.KS), case[3], noise_dtype=torch.float32)
    noise = max(float(GOLD[f"{c[0]}/noise_{q}"][np.array(c[6]) != 1].max()) for c in C.CASES for q in C.QUANTITIES)
    assert 1e-7 < noise < 1e-6
    nz = np.full(len(C.KS), noise)
    fts, locs, boxes = (out[k][0].cpu().numpy()[:len(C.KS)] for k in ("obj_fts", "obj_locs", "obj_boxes"))
    within(fts[:, :, :3], want[0][:, :, :3], nz, "xyz")
    within(fts[:, :, 3:], want[0][:, :, 3:], nz, "rgb")
    within(locs, want[1], nz, "locs")
    within(boxes, want[2], nz, "boxes")


@pytest.mark.gpu
def test_out_is_written_in_place_and_boxes_are_optional():
    case = C.CASES[0]
    objs, n = C.case_objs(case), len(C.KS)
    packed = pack(objs)
    d = C.unpack_draws(GOLD, case[0])
    a = replay(packed, d, n, 256)
    buf = {"obj_fts": torch.zeros((1, n + 2, 256, 6), device=DEV), "obj_locs": torch.zeros((1, n + 2, 6), device=DEV),
           "obj_masks": torch.zeros((1, n + 2), dtype=torch.bool, device=DEV)}
    ptrs = {k: v.untyped_storage().data_ptr() for k, v in buf.items()}
    b = replay(packed, d, n, 256, out=buf)
    for k, v in buf.items():
        assert b[k] is v and v.untyped_storage().data_ptr() == ptrs[k]
        assert torch.equal(v, a[k])
    rows = G.batch_rows(packed, ["s0"], n + 2)
    c = G.obj_processing_aug(packed, rows, 256, aug=aug_of(d), sample_idx=torch.zeros((1, n + 2, 256), dtype=torch.int32))
    assert "obj_boxes" not in c and "obj_boxes" in a
    with pytest.raises(ValueError):
        G.obj_processing_aug(packed, rows, 256, out={**buf, "obj_locs": torch.zeros((1, n + 2, 6), device=DEV).double()})
    with pytest.raises(RuntimeError):
        G.obj_processing_aug(packed, rows, 4096)              # > 2048 points per object: unsupported
    assert G.obj_processing_aug(packed, rows[:0], 64)["obj_fts"].shape == (0, n + 2, 64, 6)


def _index_coded_objects(ks):
    """Objects whose colours encode the point index (r = i & 255, g = i >> 8), as in tests/test_gpu_objects.py."""
    objs = []
    for k in ks:
        i = np.arange(k)
        pts = np.stack([i * 0.01, np.sin(i * 0.37), np.cos(i * 0.11)], 1).astype(np.float32)
        col = np.stack([i & 255, i >> 8, np.zeros_like(i)], 1).astype(np.uint8)
        objs.append((pts, col))
    return objs


def _decode(fts):
    c = np.rint((fts[..., 3:5].astype(np.float64) + 1.0) * 127.5).astype(np.int64)
    return c[..., 0] + 256 * c[..., 1]


@pytest.mark.gpu
@pytest.mark.parametrize("P", [256, 2048])
def test_device_drawn_mode(P):
    ks = [1, 5, P - 1, P, P + 1, 4097, 30000]
    packed = pack(_index_coded_objects(ks))
    rows = G.batch_rows(packed, ["s0", "s0"], len(ks) + 1)       # the same scene twice in one batch
    rng = np.random.default_rng(8)
    pub = G.draw_aug_params(C.PUBLISHED, "train", 2, len(ks) + 1, rng)
    pub.scene_rot[1] = pub.scene_rot[0]                          # ... under the same rotation
    a = G.obj_processing_aug(packed, rows, P, aug=pub, seed=7)
    b = G.obj_processing_aug(packed, rows, P, aug=pub, seed=7)
    c = G.obj_processing_aug(packed, rows, P, aug=pub, seed=8)
    assert torch.equal(a["obj_fts"], b["obj_fts"]) and torch.equal(a["obj_locs"], b["obj_locs"])
    assert not torch.equal(a["obj_fts"], c["obj_fts"])
    fts = a["obj_fts"].cpu().numpy()
    idx = _decode(fts)
    for o, k in enumerate(ks):
        for r in range(2):
            got = idx[r, o]
            assert got.min() >= 0 and got.max() < k
            if k >= P:
                assert len(set(got.tolist())) == P, (k, "np.random.choice(replace=False): distinct")
        if k > 1:
            assert not np.array_equal(idx[0, o], idx[1, o])      # two draws of the same object differ
    # device-drawn jitter: a function of (seed, row) too, and a stream of its own
    jit = G.AugParams(scene_rot=pub.scene_rot, obj_jitter=[0.01, 0.01])
    e = G.obj_processing_aug(packed, rows, P, aug=jit, seed=7)
    f = G.obj_processing_aug(packed, rows, P, aug=jit, seed=7)
    g = G.obj_processing_aug(packed, rows, P, aug=jit, seed=8)
    assert torch.equal(e["obj_fts"], f["obj_fts"]) and not torch.equal(e["obj_fts"], g["obj_fts"])
    assert np.array_equal(_decode(e["obj_fts"].cpu().numpy()), idx)          # the sampler's draws did not move
    assert not torch.equal(e["obj_locs"][0, 0], e["obj_locs"][1, 0])         # k = 1: only the noise differs
    # every real row is centred with its farthest point on the unit sphere (k = 1 without jitter is the origin)
    for out, k_min in ((a, 2), (e, 1)):
        m = out["obj_masks"]
        assert m.tolist() == [[True] * len(ks) + [False]] * 2
        real = out["obj_fts"][m][..., :3].double()
        assert real.mean(1).abs().max().item() <= 1e-6
        far = real.norm(dim=-1).max(1).values.reshape(2, len(ks)).cpu()
        sel = torch.tensor([k >= k_min for k in ks])
        assert (far[:, sel] - 1).abs().max().item() <= 1e-6
        assert far.max().item() <= 1 + 1e-6
        assert torch.all(out["obj_fts"][~m] == 1.0) and torch.all(out["obj_locs"][~m] == 0.0)


@pytest.mark.gpu
def test_device_jitter_law():
    """An object of identical points x0, jitter sigma and nothing else: x = x0 + (z - 0.5) * sigma, z ~ N(0, 1)
    (data_augmentor.py:259-260, the -0.5 shift included).  32 rows x 2048 points: N = 65536 per coordinate.
    obj_locs' centre is the row mean of x, obj_fts' xyz is (x - centre) / max_dist: dividing a row's coordinate by
    its own sample standard deviation makes it scale-free; with 2048 points per row the studentising bias of the
    statistics below (O(1 / 2048)) is a tenth of their 6-sigma bands."""
    sigma, P, B, O_ = 0.01, 2048, 4, 8
    x0 = np.array([[1.5, -2.25, 0.75]], dtype=np.float32)
    packed = pack([(np.repeat(x0, 64, 0), np.zeros((64, 3), np.uint8))])
    rows = torch.zeros((B, O_), dtype=torch.int32)
    out = G.obj_processing_aug(packed, rows, P, aug=G.AugParams(obj_jitter=[sigma] * B), seed=2024)
    N = B * O_ * P
    centre = out["obj_locs"][..., :3].double().cpu().numpy().reshape(-1, 3)
    shift = (centre - x0.astype(np.float64)).mean(0)
    print("mean(centre - x0) / sigma", shift / sigma)
    assert np.all(np.abs(shift + 0.5 * sigma) <= 6 * sigma / np.sqrt(N))
    u = out["obj_fts"][..., :3].double().cpu().numpy().reshape(-1, P, 3)
    u = u / u.std(1, keepdims=True)
    for c, v in ((1, u[..., 0]), (1, u[..., 1]), (1, u[..., 2]), (3, u)):
        p = 0.6827
        frac = np.mean(np.abs(v) < 1.0)
        kurt = np.mean(v ** 4) / np.mean(v ** 2) ** 2 - 3.0
        print(f"c={c}: within one sd {frac:.4f}, excess kurtosis {kurt:+.4f}")
        assert abs(frac - p) <= 6 * np.sqrt(p * (1 - p) / (c * N))
        assert abs(kurt) <= 6 * np.sqrt(24 / (c * N))
    for i, j in ((0, 1), (0, 2), (1, 2)):
        r = np.mean(u[..., i] * u[..., j])
        print(f"corr({i},{j}) {r:+.4f}")
        assert abs(r) <= 6 / np.sqrt(N)
    # sizes come from the jittered sample: a few sigma wide, never 0
    size = out["obj_locs"][..., 3:]
    assert size.min().item() > 4 * sigma and size.max().item() < 12 * sigma


def test_c_abi_argument_errors():
    """Host-side checks only (dummy pointers as in tests/test_capi.py): no launch happens on these paths.
    gps_obj_processing_aug(n_rows, n_points, xyz, rgb, rgb_is_u8, offsets, row_obj, sample_idx, jitter_noise,
                           noise_is_f64, seed, aug, row_aug, n_aug, fts, locs, boxes, masks, stream)"""
    f = _native.load().gps_obj_processing_aug
    assert f(0, 1024, None, None, 1, None, None, None, None, 0, 0, None, None, 0, None, None, None, None, None) == 0
    assert f(4, 0, 16, 16, 1, 16, 16, None, None, 0, 0, None, None, 0, 16, 16, None, None, None) == -1     # n_points
    assert f(-1, 8, 16, 16, 1, 16, 16, None, None, 0, 0, None, None, 0, 16, 16, None, None, None) == -1
    assert f(4, 4096, 16, 16, 1, 16, 16, None, None, 0, 0, None, None, 0, 16, 16, None, None, None) == -2  # > 2048
    assert f(4, 1024, None, 16, 1, 16, 16, None, None, 0, 0, None, None, 0, 16, 16, None, None, None) == -1  # no xyz
    assert f(4, 1024, 16, 16, 1, None, 16, None, None, 0, 0, None, None, 0, 16, 16, None, None, None) == -1  # no offsets
    assert f(4, 1024, 16, 16, 1, 16, None, None, None, 0, 0, None, None, 0, 16, 16, None, None, None) == -1  # no row_obj
    assert f(4, 1024, 16, 16, 1, 16, 16, None, None, 0, 0, None, None, 0, None, 16, None, None, None) == -1  # no obj_fts
    assert f(4, 1024, 16, 16, 1, 16, 16, None, None, 0, 0, None, None, 0, 16, None, None, None, None) == -1  # no obj_locs
    assert f(4, 1024, 8, None, 1, 16, 16, None, None, 0, 0, None, None, 0, 16, 16, None, None, None) == -1   # records % 16
    assert f(4, 1024, 16, 16, 1, 16, 16, None, None, 0, 0, 16, None, 1, 16, 16, None, None, None) == -1    # table, no index
    assert f(4, 1024, 16, 16, 1, 16, 16, None, None, 0, 0, None, 16, 0, 16, 16, None, None, None) == -1    # index, no table
    assert f(4, 1024, 16, 16, 1, 16, 16, None, None, 0, 0, 16, 16, 0, 16, 16, None, None, None) == -1      # empty table
