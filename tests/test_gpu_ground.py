"""The grounding fine-tune path on the MI355X: the kernels of csrc/gps_ground.hip against fp64 torch on the same (already
rounded) inputs, their dropout against the documented index law, the heads and og3d_loss against the reference's own
outputs (tests/golden/ground_reference_cpu.pt), and the ScanRefer-shaped train step eager vs HIP graph.

Bounds of the kernel checks (those of tests/test_gpu_qa.py::_check): fp32 outputs within 2e-5 max(1, scale), bf16 outputs
within 8e-3 scale (one bf16 rounding is 2^-8), scale = max |reference|.  The rows are drawn from randn, so that their
variances are O(1): with eps = 1e-12 the bound means nothing on near-constant rows (rstd up to 1e6)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.ground_cases import BF16_STEP_GRADS, FP32_GPU_GRADS, HEAD_CONFIGS, load_gold, run_head  # noqa: E402
from tests.test_dropout_hash import mix32, seed_fold  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-12


@pytest.fixture(scope="module")
def gold():
    return load_gold()


def _check(got, want, what):
    """fp32 results at 2e-5 max(1, scale), bf16 results at 8e-3 scale."""
    want = want.detach()
    scale = want.abs().max().item()
    err = (got.detach().double() - want).abs().max().item()
    bound = 8e-3 * scale if got.dtype == torch.bfloat16 else 2e-5 * max(1.0, scale)
    assert torch.isfinite(got).all(), what
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e} (scale {scale:.3e})"


# ---- 1: the tail kernels --------------------------------------------------------------------------------------------
def _tail_inputs(rows, d, dtype, g, seed_rows_nonpositive=()):
    h = torch.randn(rows, d, generator=g)
    h[:, 0] = 1.0 + 0.5 * h[:, 0].abs()           # one entry >= 1 and one <= -1 in every row: the variance after the ReLU is
    h[:, 1] = -h[:, 0]                            # O(1) at d = 8 too, where randn alone leaves near-constant rows
    for r in seed_rows_nonpositive:
        h[r] = -h[r].abs()
    return {"h": h.to(DEV, dtype), "gamma": (1.0 + 0.2 * torch.randn(d, generator=g)).to(DEV),
            "beta": (0.2 * torch.randn(d, generator=g)).to(DEV), "w2": (torch.randn(d, generator=g) / d ** 0.5).to(DEV),
            "b2": (0.1 * torch.randn(1, generator=g)).to(DEV), "dlogit": torch.randn(rows, generator=g).to(DEV),
            "dz16": torch.randn(rows, d, generator=g).to(DEV, torch.bfloat16)}


def _keep_mask(mode, rows, g):
    if mode == "null":
        return None
    keep = torch.zeros(rows, dtype=torch.bool)
    if mode == "one_kept":
        keep[int(torch.randint(0, rows, (1,), generator=g))] = True
    else:
        keep = torch.rand(rows, generator=g) > 0.4
        keep[0] = True
    return keep.to(DEV)


def _tail_ref(t, keep, want_logit, want_z, factor=None):
    """fp64 torch: relu, layer_norm, the explicit dropout factor (0 or 1 / (1 - p), None = no dropout), the 1-output
    Linear, masked_fill; gradients from dlogit (kept rows) and dz16."""
    h, gamma, beta, w2, b2 = (t[k].detach().double().requires_grad_(True) for k in ("h", "gamma", "beta", "w2", "b2"))
    x = F.relu(h)
    mean = x.mean(1)
    rstd = (x.var(1, unbiased=False) + EPS).rsqrt()
    z = F.layer_norm(x, (h.shape[1],), gamma, beta, EPS)
    if factor is not None:
        z = z * factor
    total, logit = 0.0, None
    if want_logit:
        raw = z @ w2 + b2
        logit = raw if keep is None else raw.masked_fill(keep.logical_not(), -float("inf"))
        contrib = raw * t["dlogit"].double()
        total = total + (contrib if keep is None else contrib[keep]).sum()
    if want_z:
        total = total + (z * t["dz16"].double()).sum()
    total.backward()
    zero = torch.zeros_like(w2)
    return {"z": z.detach(), "logit": None if logit is None else logit.detach(), "mean": mean.detach(),
            "rstd": rstd.detach(), "dpre": h.grad, "dgamma": gamma.grad, "dbeta": beta.grad,
            "dw2": zero if w2.grad is None else w2.grad, "db2": zero[:1] if b2.grad is None else b2.grad}


def _tail_run(t, keep, want_logit, want_z, p=0.0, seed=0, h=None, out=None):
    from sceneverse_amd.modules.heads.fused_mlp_head import tail_backward, tail_forward
    h = t["h"] if h is None else h
    keep8 = None if keep is None else keep.view(torch.uint8)
    w2, b2 = (t["w2"], t["b2"]) if want_logit else (None, None)
    z16, logit, mean, rstd = tail_forward(h, t["gamma"], t["beta"], EPS, p, seed, None, w2, b2, keep8, want_z16=want_z)
    dpre, dgamma, dbeta, dw2, db2 = tail_backward(h, t["gamma"], t["beta"], mean, rstd, p, seed, None, w2, keep8,
                                                  t["dlogit"] if want_logit else None, t["dz16"] if want_z else None, out=out)
    return {"z": z16, "logit": logit, "mean": mean, "rstd": rstd, "dpre": dpre, "dgamma": dgamma, "dbeta": dbeta,
            "dw2": dw2, "db2": db2}


def _compare(got, ref, keep, dtype, what):
    for k, v in got.items():
        if v is None:
            continue
        if k == "logit" and keep is not None:
            assert bool((v[~keep] == -float("inf")).all()), what + ": masked logits must be exactly -inf"
            if keep.any():
                _check(v[keep], ref[k][keep], f"{what} logit")
            continue
        if k == "z":
            assert v.dtype == torch.bfloat16
        if k == "dpre":
            assert v.dtype == dtype
        _check(v, ref[k], f"{what} {k}")


def _same_bits(a, b, what):
    for k in a:
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), f"{what}: two runs differ in {k}"


MODES = {"logit": (True, False), "hidden": (False, True), "both": (True, True)}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("d", [8, 64, 384, 768, 1024])
def test_mlp_tail_matches_fp64(d, dtype):
    g = torch.Generator().manual_seed(4000 + d)
    for rows in (1, 3, 65, 257):
        t = _tail_inputs(rows, d, dtype, g)
        for mode, (want_logit, want_z) in MODES.items():
            for kmode in (("null", "random", "one_kept") if want_logit else ("null",)):
                keep = _keep_mask(kmode, rows, g)
                what = f"rows={rows} d={d} {dtype} {mode} keep={kmode}"
                a = _tail_run(t, keep, want_logit, want_z)
                b = _tail_run(t, keep, want_logit, want_z)
                _same_bits(a, b, what)
                ref = _tail_ref(t, keep, want_logit, want_z)
                _compare(a, ref, keep, dtype, what)
                if keep is not None and not want_z:      # masked rows: no gradient at all, whatever dlogit holds there
                    assert float(a["dpre"][~keep].float().abs().max()) == 0.0 if (~keep).any() else True, what
                    t2 = dict(t, dlogit=torch.where(keep, t["dlogit"], torch.full_like(t["dlogit"], float("nan"))))
                    c = _tail_run(t2, keep, want_logit, want_z)
                    for k in ("dpre", "dgamma", "dbeta", "dw2", "db2"):
                        assert torch.equal(a[k], c[k]), f"{what}: a masked row's dlogit reached {k}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_mlp_tail_reads_pitched_rows_in_place(dtype):
    """h as a column slice of a wider tensor (row pitch d + 8), dpre into such a slice: nothing lands in the pad columns."""
    from sceneverse_amd.modules.heads import fused_mlp_head
    g = torch.Generator().manual_seed(91)
    for rows, d in ((65, 384), (3, 8), (5, 1024)):
        t = _tail_inputs(rows, d, dtype, g)
        wide = torch.randn(rows, d + 8, generator=g).to(DEV, dtype)
        wide[:, :d] = t["h"]
        hv = wide[:, :d]
        assert fused_mlp_head._rows_view(hv) is hv and hv.stride(0) == d + 8
        out_wide = torch.full((rows, d + 8), 7.0, device=DEV, dtype=dtype)
        keep = _keep_mask("random", rows, g)
        got = _tail_run(t, keep, True, True, h=hv, out=out_wide[:, :d])
        what = f"pitched rows={rows} d={d} {dtype}"
        assert bool((out_wide[:, d:] == 7.0).all()), what
        _compare(got, _tail_ref(t, keep, True, True), keep, dtype, what)


@pytest.mark.parametrize("p", [0.0, 0.3])
def test_mlp_tail_row_without_a_positive_entry(p):
    """The deliberate edge: a row that is entirely <= 0 has variance 0 after the ReLU, rstd = 1e6 at eps 1e-12.  Its
    output is beta under the dropout mask, its input gradient 0, everything finite."""
    g = torch.Generator().manual_seed(5)
    rows, d, seed = 3, 384, 77
    for dtype in (torch.bfloat16, torch.float32):
        t = _tail_inputs(rows, d, dtype, g, seed_rows_nonpositive=(1,))
        got = _tail_run(t, None, True, True, p=p, seed=seed)
        for k, v in got.items():
            assert torch.isfinite(v).all(), (k, dtype)
        factor = _factor(rows, d, p, seed)
        want = (t["beta"] * factor[1].float()).to(torch.bfloat16)      # one fp32 product, one rounding: the kernel's
        assert torch.equal(got["z"][1], want), dtype
        assert float(got["dpre"][1].float().abs().max()) == 0.0
        assert abs(float(got["rstd"][1]) - 1e6) <= 1e6 * 1e-3 and float(got["mean"][1]) == 0.0
        ref = _tail_ref(t, None, True, True, factor=factor if p else None)
        for k in ("logit", "dgamma", "dbeta", "dw2", "db2"):
            _check(got[k], ref[k], f"nonpositive row p={p} {dtype} {k}")
        _check(got["dpre"][[0, 2]], ref["dpre"][[0, 2]], f"nonpositive row p={p} {dtype} dpre")


# ---- 2: dropout against the documented index law ---------------------------------------------------------------------
def _factor(rows, d, p, seed):
    """Element (r, c) draws mix32((r d + c) ^ seed_fold(seed)) (indices below 2^32), is kept iff that is >=
    (uint32)(p 2^32) with p as a float32, and is scaled by the float32 1 / (1 - p)."""
    if p == 0.0:
        return torch.ones(rows, d, dtype=torch.float64, device=DEV)
    idx = np.arange(rows * d, dtype=np.uint64)
    bits = mix32(idx ^ seed_fold(seed))
    thr = np.uint64(int(float(np.float32(p)) * 4294967296.0))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return torch.from_numpy((bits >= thr).astype(np.float64) * scale).view(rows, d).to(DEV)


@pytest.mark.parametrize("rows,d", [(65, 384), (3, 1024)])
def test_mlp_tail_dropout_follows_the_documented_stream(rows, d):
    g = torch.Generator().manual_seed(rows + d)
    p, seed = 0.3, (5 << 32) + 12345
    factor = _factor(rows, d, p, seed)
    assert 0.6 < float((factor > 0).double().mean()) < 0.8
    for dtype in (torch.bfloat16, torch.float32):
        t = _tail_inputs(rows, d, dtype, g)
        keep = _keep_mask("random", rows, g)
        what = f"dropout rows={rows} d={d} {dtype}"
        a = _tail_run(t, keep, True, True, p=p, seed=seed)
        _same_bits(a, _tail_run(t, keep, True, True, p=p, seed=seed), what)
        _compare(a, _tail_ref(t, keep, True, True, factor=factor), keep, dtype, what)      # backward draws the same mask
        assert torch.equal(a["z"] == 0, factor == 0), what
        other = _tail_run(t, keep, True, True, p=p, seed=seed + 1)
        assert not torch.equal(other["z"], a["z"]), what + ": another seed, the same mask"


# ---- 3: og3d cross entropy -------------------------------------------------------------------------------------------
def _ce_case(B, O, g, pitched):
    x = 3 * torch.randn(B, O + (3 if pitched else 0), generator=g)
    logical = x[:, :O]
    dead = torch.rand(B, O, generator=g) < 0.3
    dead[torch.arange(B), torch.randint(0, O, (B,), generator=g)] = False          # never a whole row
    logical[dead] = -float("inf")
    tgt = torch.empty(B, dtype=torch.long)
    for b in range(B):
        live = (~dead[b]).nonzero().flatten()
        tgt[b] = live[-1] if b % 2 == 0 else live[int(torch.randint(0, len(live), (1,), generator=g))]
    if B >= 3:
        tgt[1] = -100
    return x.to(DEV), tgt.to(DEV), dead.to(DEV)


@pytest.mark.parametrize("O", [1, 7, 64, 65, 80, 512])
def test_og3d_ce_matches_fp64(O):
    from sceneverse_amd.optim.loss.fused_og3d import og3d_ce, og3d_ce_usable
    g = torch.Generator().manual_seed(600 + O)
    gout = torch.tensor(0.75, device=DEV)
    for B in (1, 3, 65):
        for pitched in (False, True):
            for tgt_shape in ((B,), (B, 1)):
                wide, tgt, dead = _ce_case(B, O, g, pitched)
                what = f"B={B} O={O} pitched={pitched} target{tgt_shape}"
                runs = []
                for _ in range(2):
                    w = wide.clone().requires_grad_(True)
                    x = w[:, :O]
                    assert og3d_ce_usable(x, tgt.view(tgt_shape)), what
                    loss = og3d_ce(x, tgt.view(tgt_shape))
                    loss.backward(gout)
                    runs.append((loss.detach(), w.grad))
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what
                x64 = wide[:, :O].double().requires_grad_(True)
                ref = F.cross_entropy(x64, tgt)
                ref.backward(gout.double())
                loss, grad = runs[0]
                assert loss.dtype == torch.float32 and loss.dim() == 0
                _check(loss, ref, what + " loss")
                _check(grad[:, :O], x64.grad, what + " dlogits")
                assert float(grad[:, :O][dead].abs().max() if dead.any() else 0.0) == 0.0, what
                assert float(grad[:, O:].abs().max() if pitched else 0.0) == 0.0, what
                if B >= 3:
                    assert float(grad[1].abs().max()) == 0.0, what + ": the ignored row"


def test_og3d_ce_row_of_all_minus_inf_is_nan_like_torch():
    from sceneverse_amd.optim.loss.fused_og3d import og3d_ce
    x = torch.randn(3, 7, device=DEV)
    x[1] = -float("inf")
    tgt = torch.tensor([0, 3, 6], device=DEV)
    xs = x.clone().requires_grad_(True)
    loss = og3d_ce(xs, tgt)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isnan(loss) and torch.isnan(F.cross_entropy(x, tgt))
    assert float(xs.grad[1].abs().max()) == 0.0 and torch.isfinite(xs.grad[[0, 2]]).all()


def test_og3d_loss_switch_and_fallbacks():
    """`_FUSED_OG3D = False` and logits the kernel does not serve (more than 512 objects) keep F.cross_entropy."""
    from sceneverse_amd.optim.loss import loss as L
    from sceneverse_amd.pointnet2 import _ext
    g = torch.Generator().manual_seed(1)
    x, tgt = torch.randn(4, 80, generator=g).to(DEV), torch.randint(0, 80, (4, 1), generator=g).to(DEV)
    with _fused_loss(True):
        _ext.profile_start()
        native = L.og3d_loss({"og3d_logits": x, "tgt_object_id": tgt})
        assert any(k.startswith("og3d_ce") for k in _ext.profile_stop())
    with _fused_loss(False):
        _ext.profile_start()
        plain = L.og3d_loss({"og3d_logits": x, "tgt_object_id": tgt})
        assert not any(k.startswith("og3d_ce") for k in _ext.profile_stop())
    torch.testing.assert_close(native, plain, rtol=1e-5, atol=1e-5)
    big = torch.randn(2, 600, generator=g).to(DEV)
    t2 = torch.tensor([[5], [599]], device=DEV)
    with _fused_loss(True):
        torch.testing.assert_close(L.og3d_loss({"og3d_logits": big, "tgt_object_id": t2}), F.cross_entropy(big, t2.squeeze(1)))


# ---- 4: heads + loss against the reference ---------------------------------------------------------------------------
class _fused_loss:
    """`loss._FUSED_OG3D` for the duration of a block (the native og3d_loss ships selectable and off)."""

    def __init__(self, flag):
        self.flag = flag

    def __enter__(self):
        from sceneverse_amd.optim.loss import loss as L
        self.old, L._FUSED_OG3D = L._FUSED_OG3D, self.flag

    def __exit__(self, *exc):
        from sceneverse_amd.optim.loss import loss as L
        L._FUSED_OG3D = self.old
        return False


class _backend:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from sceneverse_amd.modules.heads import grounding_head
        grounding_head.set_ground_backend(self.name)

    def __exit__(self, *exc):
        from sceneverse_amd.modules.heads import grounding_head
        grounding_head.set_ground_backend("auto")
        return False


def _count_native(fn):
    """Run fn under the launch profiler of the native ops; -> names of the ops it launched."""
    from sceneverse_amd.pointnet2 import _ext
    _ext.profile_start()
    try:
        fn()
    finally:
        seen = _ext.profile_stop()
    return set(k.split("(")[0] for k in seen)


_HEAD_OPS = {"mlp_tail_forward", "mlp_tail_backward", "og3d_ce_forward"}


def _torch_argmax(name, autocast):
    """argmax of the og3d logits of the torch composition on the golden inputs."""
    with _backend("torch"), _fused_loss(False):
        bounds = BF16_STEP_GRADS if autocast else FP32_GPU_GRADS
        return run_head(DEV, load_gold(), name, 6e-2 if autocast else 2e-3, bounds, autocast=autocast,
                        ltol=3e-2 if autocast else None).argmax(1)


@pytest.mark.parametrize("name", sorted(HEAD_CONFIGS))
def test_ground_head_gpu_fp32_matches_reference(gold, name):
    og3d = run_head(DEV, gold, name, 2e-3, FP32_GPU_GRADS)
    assert og3d.dtype == torch.float32
    with _backend("hip"), _fused_loss(True):
        ops = _count_native(lambda: run_head(DEV, gold, name, 2e-3, FP32_GPU_GRADS))
    assert _HEAD_OPS <= ops, ops
    assert torch.equal(og3d.argmax(1), _torch_argmax(name, False))


@pytest.mark.parametrize("name", sorted(HEAD_CONFIGS))
def test_ground_head_gpu_bf16_matches_reference(gold, name):
    og3d = run_head(DEV, gold, name, 6e-2, BF16_STEP_GRADS, autocast=True, ltol=3e-2)
    assert og3d.dtype == torch.float32                    # fp32 under autocast too (the composition gives bf16)
    with _backend("hip"), _fused_loss(True):
        ops = _count_native(lambda: run_head(DEV, gold, name, 6e-2, BF16_STEP_GRADS, autocast=True, ltol=3e-2))
    assert _HEAD_OPS <= ops, ops
    assert any(k.startswith("gemm") for k in ops), ops              # the first Linears ran on the library's GEMMs
    assert torch.equal(og3d.argmax(1), _torch_argmax(name, True))


def test_hip_backend_raises_on_a_call_the_library_does_not_serve():
    from sceneverse_amd.modules.heads.grounding_head import GroundHead
    from sceneverse_amd.modules.utils import get_mlp_head
    head = GroundHead(None, input_size=768, hidden_size=384, dropout=0.0).to(DEV).eval()
    head.og3d_head = get_mlp_head(768, 100, 1).to(DEV)        # 100: not a multiple of 8
    x, m = torch.randn(2, 7, 768, device=DEV), torch.ones(2, 7, dtype=torch.bool, device=DEV)
    assert head(x, m).shape == (2, 7)                         # "auto": the torch composition
    with _backend("hip"), pytest.raises(RuntimeError, match="unsupported"):
        head(x, m)


def test_head_reads_dropout_p_and_training_at_call_time():
    """p is zeroed after construction by existing tests: a training-mode call must then equal the eval-mode call; with
    p = 0.3 in training mode it must differ, and stay finite."""
    from sceneverse_amd.modules.heads.grounding_head import GroundHead
    head = GroundHead(None, input_size=768, hidden_size=384, dropout=0.3).to(DEV)
    x, m = torch.randn(4, 16, 768, device=DEV), torch.ones(4, 16, dtype=torch.bool, device=DEV)
    ev = head.eval()(x, m)
    dropped = head.train()(x, m)
    assert torch.isfinite(dropped).all() and not torch.equal(dropped, ev)
    for mod in head.modules():
        if isinstance(mod, nn.Dropout):
            mod.p = 0.0
    assert torch.equal(head.train()(x, m), ev)


# ---- 5: the train step: eager vs HIP graph ---------------------------------------------------------------------------
def _engine(graph, dropout_off, seed=7):
    from sceneverse_amd.engine import GPSTrainStep
    from sceneverse_amd.modules.layers.transformers import MultiheadSelfAttention
    from tests.util import gps_cfg, lang_dir
    cfg = gps_cfg(lang_dir(0), heads="ground", use_scene_cap=False)
    cfg.solver.sched.args.warmup_steps = 4
    st = GPSTrainStep(cfg, device=DEV, ddp=False, graph=graph, graph_warmup=2, seed=seed)
    if dropout_off:
        for m in st.model.modules():
            if isinstance(m, nn.Dropout):
                m.p = 0.0
            if isinstance(m, MultiheadSelfAttention):
                m.dropout = 0.0
            if hasattr(m, "attention_probs_dropout_prob"):
                m.attention_probs_dropout_prob = 0.0
            if hasattr(m, "dropout_prob"):
                m.dropout_prob = 0.0
    return st


def test_ground_train_step_graph_matches_eager_and_learns():
    """GPSTrainStep on the ScanRefer-shaped config (GroundHeadV1 768 / 384 / 607, og3d_loss), 4 scenes x 16 objects, 5
    steps on one batch, dropout zeroed so both runs are deterministic functions of the weights: the captured step gives
    the eager losses within 2e-3 relative, `_graph` is set, the loss falls, and the native head and loss ran."""
    from sceneverse_amd.data.synthetic import synth_batch
    batch = synth_batch(4, n_obj=16, seed=23, min_real=5, device=DEV)
    runs = {}
    for graph in (False, True):
        with _fused_loss(True):                           # the native loss is captured too
            st = _engine(graph, True)
            losses = []
            if not graph:
                ops = _count_native(lambda: losses.append(st.step(dict(batch))[0].item()))
                assert _HEAD_OPS <= ops, ops
            while len(losses) < 5:
                total, parts = st.step(dict(batch))
                losses.append(total.item())
        assert set(parts) >= {"og3d_loss", "total_loss"}
        if graph:
            assert st._graph is not None                  # steps 3.. were graph replays
        runs[graph] = losses
    eager, graphed = runs[False], runs[True]
    assert all(x == x for x in eager + graphed), runs
    for a, b in zip(eager, graphed):
        assert abs(a - b) <= 2e-3 * abs(a), runs
    assert eager[-1] < eager[0] and graphed[-1] < graphed[0], runs


def test_ground_train_step_with_dropout_is_finite_and_seeded():
    from sceneverse_amd.data.synthetic import synth_batch
    from sceneverse_amd.modules.layers import fused_attention
    batch = synth_batch(4, n_obj=16, seed=23, min_real=5, device=DEV)
    dev = torch.device("cuda", torch.cuda.current_device())
    state = fused_attention.snapshot_seed_state(dev)      # the device's dropout seed stream outlives an engine
    losses = []
    for _ in range(2):
        fused_attention.restore_seed_state(dev, state)
        losses.append(_engine(False, False, seed=11).step(dict(batch))[0].item())
    assert losses[0] == losses[0] and abs(losses[0]) < 1e4, losses
    assert losses[0] == losses[1], losses
