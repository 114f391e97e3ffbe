"""The distinct-sample form of the fused set-abstraction levels (gps_sa_mlp_set_distinct(2): both levels) against the dense
form of the same launches (every one of the 32 slots of a group through the MLP) and against an fp64 torch formulation.

Slot c > 0 of a group is dropped iff idx[c] == idx[0] -- whatever idx holds: the indices are built by hand here, not by
gps_ball_query.  max over a set = max over the set with repeats, so the two forms must pool the same values
(torch.equal) and the same bits apart from the sign of a zero.

Tolerances: 1e-4 * max|ref| against fp64 for the split-bf16 triple product (tests/test_gpu_sa_fused.py); for the
single-product mode the tolerance stated there, max|diff| <= 2e-2 * max|ref| and relative L2 <= 1e-2."""
import os
import sys

import pytest
import torch

from sceneverse_amd.pointnet2 import _ext

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import sa_mlp_digests  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (b, n, npoint, C, channels): the SA2 form (streamed weights, several objects per workgroup; 5 objects are no multiple
# of any objects-per-workgroup > 1) and the SA1 form (resident weights; 5 groups are no multiple of the 8 waves)
SHAPES = {"sa2": (5, 32, 16, 128, (128, 128, 256)), "sa1": (3, 64, 5, 3, (64, 64, 128))}
PATTERNS = ["one_distinct", "all_distinct", "mixed", "not_a_prefix", "extent"]
SENTINEL = -123.5


def _group(g, n, count, first):
    """32 slots: `count` distinct indices starting with `first`, the rest filled with `first` (the ball query's form)."""
    perm = torch.randperm(n, generator=g)
    perm = perm[perm != first][:count - 1]
    return torch.cat([torch.tensor([first]), perm, torch.full((32 - count,), first)]).to(torch.int32)


def _idx(pattern, b, n, npoint, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.empty(b, npoint, 32, dtype=torch.int32)
    if pattern == "one_distinct":
        idx[:] = torch.randint(0, n, (b, npoint, 1), generator=g, dtype=torch.int32)
    elif pattern == "all_distinct":
        for o in range(b):
            for j in range(npoint):
                idx[o, j] = torch.randperm(n, generator=g)[:32].to(torch.int32)
    elif pattern in ("mixed", "extent"):
        # per-object totals that are no multiples of 32, groups straddling the 32-column tiles
        cycle = [5, 31, 1, 32, 2, 30, 7, 17, 3, 29, 9, 13, 1, 27, 4, 11]
        for o in range(b):
            for j in range(npoint):
                idx[o, j] = _group(g, n, cycle[(3 * o + j) % len(cycle)], int(torch.randint(0, n, (1,), generator=g)))
        if npoint == 16:
            # object 1: 15 full groups + 31 = 511 columns (> 256: a second streamed round); object 2: 16 + 3 = 19 columns (< 32)
            for j in range(npoint):
                idx[1, j] = _group(g, n, 32 if j != 6 else 31, j)
                idx[2, j] = _group(g, n, 1 if j not in (4, 9, 15) else 2, (5 * j) % n)
    elif pattern == "not_a_prefix":
        for o in range(b):
            for j in range(npoint):
                first = int(torch.randint(0, n, (1,), generator=g))
                row = torch.full((32,), first, dtype=torch.int32)
                others = torch.randperm(n, generator=g)
                others = others[others != first]
                if (o + j) % 2 == 0:        # [3, 3, 7, 3, 9, 3, ...]: fillers between the kept slots
                    row[2::2] = others[:15].to(torch.int32)
                else:                        # [3, 7, 7, 5, 5, 5, 3, 8, ...]: a NON-first index repeats -- kept and computed
                    row[1:3] = int(others[0])
                    row[3:6] = int(others[1])
                    row[7] = int(others[2])
                    row[31] = int(others[0])
                idx[o, j] = row
    return idx


def _inputs(level, seed):
    b, n, npoint, c, ch = SHAPES[level]
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(b, n, 3, generator=g) * 2 - 1
    new_xyz = torch.rand(b, npoint, 3, generator=g) * 2 - 1
    feats = torch.randn(b, c, n, generator=g)
    ws, shifts, c_in = [], [], 3 + c
    for c_out in ch:
        ws.append(torch.randn(c_out, c_in, generator=g) / c_in ** 0.5)
        shifts.append(torch.randn(c_out, generator=g) * 0.1)
        c_in = c_out
    return xyz, new_xyz, feats, ws, shifts


def _reference(xyz, new_xyz, feats, idx, ws, shifts):
    """fp64: gather, subtract the centre, three matmul + shift + ReLU, max over the 32 slots -> (b, c3, npoint)."""
    b, npoint = idx.shape[:2]
    xyz, new_xyz, feats = xyz.double(), new_xyz.double(), feats.double()
    ii = idx.long().reshape(b, -1)
    gx = torch.gather(xyz, 1, ii[..., None].expand(-1, -1, 3)).reshape(b, npoint, 32, 3) - new_xyz[:, :, None, :]
    gf = torch.gather(feats, 2, ii[:, None, :].expand(-1, feats.shape[1], -1)).reshape(b, -1, npoint, 32)
    x = torch.cat([gx.permute(0, 3, 1, 2), gf], 1)                      # (b, 3 + c, npoint, 32)
    for w, s in zip(ws, shifts):
        x = torch.relu(torch.einsum("oc,bcjk->bojk", w.double(), x) + s.double()[None, :, None, None])
    return x.max(dim=3).values


def _level_inputs(level):
    return _inputs(level, 7 + list(SHAPES).index(level))


def _build_cases():
    """inputs, packed weights and the fp64 reference of every (level, pattern)."""
    out = {}
    for li, level in enumerate(SHAPES):
        b, n, npoint, c, ch = SHAPES[level]
        xyz, new_xyz, feats, ws, shifts = _level_inputs(level)
        dev = [t.to(DEV) for t in (xyz, new_xyz, feats)]
        wpack = _ext.sa_mlp_pack([w.to(DEV) for w in ws], [s.to(DEV) for s in shifts], "bf16x3")
        for pi, pattern in enumerate(PATTERNS):
            idx = _idx(pattern, b, n, npoint, 100 * li + pi)
            out[level, pattern] = (dev, idx.to(DEV), wpack, ch, _reference(xyz, new_xyz, feats, idx, ws, shifts).float())
    return out


@pytest.fixture(scope="module")
def cases():
    """computed once, never modified"""
    return _build_cases()


def _run(level, case, entry, extent):
    (xyz, new_xyz, feats), idx, wpack, ch, _ = case
    b, n, npoint, c, _ = SHAPES[level]
    import sceneverse_amd._native as _native
    lib = _native.load()
    out = torch.full((b, ch[2], npoint), SENTINEL, dtype=torch.float32, device=DEV)
    n_dev = torch.tensor([extent], dtype=torch.int32, device=DEV) if extent is not None else None
    stream = torch.cuda.current_stream().cuda_stream
    with _ext.object_extent(n_dev):
        if entry == "pm":
            pm = feats.transpose(1, 2).contiguous()                       # (b, n, c) point-major
            st = lib.gps_sa_mlp_forward_bf16x3_pm(b, n, npoint, 32, c, *ch, xyz.data_ptr(), new_xyz.data_ptr(), pm.data_ptr(), c,
                                                  idx.data_ptr(), wpack.data_ptr(), out.data_ptr(), stream)
        else:
            st = lib.gps_sa_mlp_forward_bf16x3(b, n, npoint, 32, c, *ch, xyz.data_ptr(), new_xyz.data_ptr(), feats.data_ptr(),
                                               idx.data_ptr(), wpack.data_ptr(), out.data_ptr(), stream)
    _native.check(st, "sa_mlp_forward")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("products", [3, 1])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("level,entry", [("sa2", "cm"), ("sa1", "cm"), ("sa1", "pm")])
def test_distinct_form_pools_what_the_dense_form_pools(cases, level, entry, pattern, products):
    import sceneverse_amd._native as _native
    lib = _native.load()
    case = cases[level, pattern]
    b = SHAPES[level][0]
    extent = b - 1 if pattern == "extent" else None       # cuts the last workgroup of the several-objects form in two
    live = b if extent is None else extent
    ref = case[4].to(DEV)
    try:
        lib.gps_sa_mlp_set_products(products)
        lib.gps_sa_mlp_set_distinct(2)                                  # every level on its distinct samples
        got = _run(level, case, entry, extent)
        lib.gps_sa_mlp_set_distinct(0)
        dense = _run(level, case, entry, extent)
    finally:
        lib.gps_sa_mlp_set_products(3)
        lib.gps_sa_mlp_set_distinct(1)
    # objects past the device-side extent: neither form wrote them
    assert (got[live:] == SENTINEL).all() and (dense[live:] == SENTINEL).all()
    got, dense, ref = got[:live], dense[:live], ref[:live]
    assert torch.equal(got, dense)
    gb, db = got.view(torch.int32), dense.view(torch.int32)
    differ = gb != db
    assert ((got[differ] == 0) & (dense[differ] == 0)).all()            # bit-equal apart from the sign of a zero
    scale = ref.abs().max().item()
    for name, t in (("distinct", got), ("dense", dense)):
        err = (t - ref).abs().max().item()
        rel = ((t - ref).norm() / ref.norm()).item()
        print(f"[sa-distinct] {level}/{entry}/{pattern}/products={products} {name}: max|diff|/max|ref| = {err / scale:.3e}, rel L2 = {rel:.3e}")
        if products == 3:
            assert err <= 1e-4 * scale, (name, err, scale)
        else:
            assert err <= 2e-2 * scale and rel <= 1e-2, (name, err / scale, rel)


def test_switch_reports_and_restores_its_setting():
    try:
        _ext.sa_mlp_set_distinct(1)                                      # whatever an earlier failure left behind
        assert _ext.sa_mlp_set_distinct(0) == 1
        assert _ext.sa_mlp_set_distinct(2) == 0
        assert _ext.sa_mlp_set_distinct(7) == 2                          # anything else = query
        assert _ext.sa_mlp_set_distinct(-1) == 2
    finally:
        _ext.sa_mlp_set_distinct(1)


def test_library_default_is_the_streamed_level_only():
    """A fresh process: the library starts with setting 1 (SA2 distinct, SA1 dense)."""
    import subprocess
    import sys
    code = "from sceneverse_amd import _native; print(_native.load().gps_sa_mlp_set_distinct(-1))"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    assert out.stdout.strip().splitlines()[-1] == "1"


def test_default_setting_runs_the_streamed_level_on_distinct_samples(cases):
    """Setting 1 (the default) and setting 2 launch the same kernel for the SA2 form: the same bits, and a pooled zero is
    +0 (the dense kernel may leave -0)."""
    case = cases["sa2", "mixed"]
    try:
        _ext.sa_mlp_set_distinct(1)
        one = _run("sa2", case, "cm", None)
        _ext.sa_mlp_set_distinct(2)
        two = _run("sa2", case, "cm", None)
    finally:
        _ext.sa_mlp_set_distinct(1)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    assert not (one.view(torch.int32) == -2 ** 31).any()


def test_shape_too_large_for_the_column_list_runs_the_dense_kernel():
    """SA2 form with n = 64, npoint = 72: the dense kernel needs 156 KB of LDS, the distinct form's column list and pooled-row
    pitch would need 166 KB even for one object per workgroup -- the default setting must launch the dense kernel, not fail."""
    b, n, npoint, c, ch = 2, 64, 72, 128, (128, 128, 256)
    g = torch.Generator().manual_seed(5)
    xyz = (torch.rand(b, n, 3, generator=g) * 2 - 1).to(DEV)
    new_xyz = (torch.rand(b, npoint, 3, generator=g) * 2 - 1).to(DEV)
    feats = torch.randn(b, c, n, generator=g).to(DEV)
    idx = torch.randint(0, n, (b, npoint, 32), generator=g, dtype=torch.int32).to(DEV)
    ws, shifts, c_in = [], [], 3 + c
    for c_out in ch:
        ws.append((torch.randn(c_out, c_in, generator=g) / c_in ** 0.5).to(DEV))
        shifts.append((torch.randn(c_out, generator=g) * 0.1).to(DEV))
        c_in = c_out
    wpack = _ext.sa_mlp_pack(ws, shifts, "bf16x3")
    try:
        _ext.sa_mlp_set_distinct(0)
        dense = _ext.sa_mlp_forward(xyz, new_xyz, feats, idx, wpack, ch, "bf16x3")
        _ext.sa_mlp_set_distinct(2)
        got = _ext.sa_mlp_forward(xyz, new_xyz, feats, idx, wpack, ch, "bf16x3")
    finally:
        _ext.sa_mlp_set_distinct(1)
    assert torch.equal(got.view(torch.int32), dense.view(torch.int32))
    ref = _reference(xyz.cpu(), new_xyz.cpu(), feats.cpu(), idx.cpu(), [w.cpu() for w in ws], [s.cpu() for s in shifts]).float()
    assert (got.cpu() - ref).abs().max().item() <= 1e-4 * ref.abs().max().item()


def test_frozen_digests_cover_every_case():
    assert sa_mlp_digests.PATTERNS == PATTERNS
    assert sorted(sa_mlp_digests.load()) == sorted(sa_mlp_digests.keys())


@pytest.mark.parametrize("key", sa_mlp_digests.keys())
def test_output_bits_are_the_frozen_ones(cases, key):
    """tests/golden/sa_mlp_digests.json (tools/sa_mlp_digests.py): SHA-256 of the raw output, sentinel rows included, of the
    dense and the distinct bf16x3 kernels on every case above and of the fp32 kernel on four of them.  Both forms are
    deterministic -- fixed MFMA order, order-independent integer max -- so a mismatch is a change of arithmetic to explain
    (a term moved across the split8 subtraction, another accumulator initialisation), never a tolerance."""
    assert sa_mlp_digests.compute(key, cases, sys.modules[__name__]) == sa_mlp_digests.load()[key]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
def test_second_device_of_the_process_gets_its_own_lds_grant():
    """SA1 form with n = 1024, npoint = 32: 104 KB of dynamic LDS, above the 64 KiB a kernel has without opting in.  The
    opt-in belongs to the (kernel, device) pair: the launch on cuda:1 after one on cuda:0 must be granted too."""
    b, n, npoint, c, ch = 2, 1024, 32, 3, (64, 64, 128)
    g = torch.Generator().manual_seed(11)
    xyz = torch.rand(b, n, 3, generator=g) * 2 - 1
    new_xyz = torch.rand(b, npoint, 3, generator=g) * 2 - 1
    feats = torch.randn(b, c, n, generator=g)
    idx = torch.randint(0, n, (b, npoint, 32), generator=g, dtype=torch.int32)
    ws, shifts, c_in = [], [], 3 + c
    for c_out in ch:
        ws.append(torch.randn(c_out, c_in, generator=g) / c_in ** 0.5)
        shifts.append(torch.randn(c_out, generator=g) * 0.1)
        c_in = c_out
    outs = []
    for d in ("cuda:0", "cuda:1"):
        wpack = _ext.sa_mlp_pack([w.to(d) for w in ws], [s.to(d) for s in shifts], "bf16x3")
        out = _ext.sa_mlp_forward(xyz.to(d), new_xyz.to(d), feats.to(d), idx.to(d), wpack, ch, "bf16x3")
        torch.cuda.synchronize(d)
        outs.append(out.cpu())
    assert torch.equal(outs[0], outs[1])
