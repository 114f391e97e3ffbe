"""The question-answering fine-tune path on the MI355X: the three native ops of csrc/gps_qa.hip /
gps_contrastive.hip against fp64 torch on the same (already rounded) inputs, the head, the losses and the whole model
against the reference's own outputs (tests/golden/qa_reference_cpu.pt), and the ScanQA train step eager vs HIP graph.

Bounds of the kernel checks: fp32 outputs within 2e-5 max(1, scale) (fp32 accumulation over <= 512 * 1024 terms),
bf16 outputs within 8e-3 scale (one bf16 rounding is 2^-8), scale = max |reference|."""
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.qa_cases import (BF16_STEP_GRADS, FP32_GPU_GRADS, HEAD_CONFIGS, as_qa_cfg, load_gold, run_head,  # noqa: E402
                            run_model)

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


# ---- 1a: AttFlat pooling --------------------------------------------------------------------------------------------
def _keep(mode, B, T, g):
    if mode == "null":
        return None
    keep = torch.ones(B, T, dtype=torch.bool)
    if mode == "one_valid":
        keep[:] = False
        keep[torch.arange(B), torch.randint(0, T, (B,), generator=g)] = True
    elif mode == "empty_row":
        keep = torch.rand(B, T, generator=g) > 0.4
        keep[:, 0] = True
        keep[0] = False                                   # no valid token: uniform 1 / T weights, no logit gradient
    return keep


def _attflat_ref(x, h, w2, b2, keep, dpooled):
    x, h, w2, b2 = (t.detach().double().requires_grad_(True) for t in (x, h, w2, b2))
    logit = h @ w2.t() + b2
    if keep is not None:
        logit = logit.masked_fill(keep.logical_not().unsqueeze(2), -1e9)
    att = F.softmax(logit, dim=1)
    pooled = torch.einsum("btg,btd->bgd", att, x).flatten(1)
    pooled.backward(dpooled.double())
    return pooled, att, x.grad, h.grad, w2.grad, b2.grad


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("T", [1, 7, 65, 130, 512])
def test_attflat_pool_matches_fp64(T, dtype):
    from sceneverse_amd.modules.heads.fused_attflat import attflat_pool, attflat_pool_usable
    g = torch.Generator().manual_seed(1000 + T)
    for B in (1, 3):
        for G in (1, 2):
            for D, M in ((64, 8), (768, 256)):
                for mode in ("null", "all_valid", "one_valid", "empty_row"):
                    x = torch.randn(B, T, D, generator=g).to(DEV, dtype)
                    h = torch.randn(B, T, M, generator=g).to(DEV, dtype)
                    w2 = (torch.randn(G, M, generator=g) / M ** 0.5).to(DEV)
                    b2 = (0.1 * torch.randn(G, generator=g)).to(DEV)
                    keep = _keep(mode, B, T, g)
                    keep = None if keep is None else keep.to(DEV)
                    dpooled = torch.randn(B, G * D, generator=g).to(DEV)
                    what = f"B={B} T={T} G={G} D={D} M={M} keep={mode}"
                    assert attflat_pool_usable(x, h, w2, keep), what
                    runs = []
                    for _ in range(2):
                        xs, hs, ws, bs = (t.clone().requires_grad_(True) for t in (x, h, w2, b2))
                        pooled, att = attflat_pool(xs, hs, ws, bs, keep, return_att=True)
                        pooled.backward(dpooled)
                        runs.append((pooled.detach(), att, xs.grad, hs.grad, ws.grad, bs.grad))
                    for a, b in zip(*runs):
                        assert torch.equal(a, b), what + ": two runs differ"
                    ref = _attflat_ref(x, h, w2, b2, keep, dpooled)
                    for name, got, want in zip(("pooled", "att", "dx", "dh", "dw2", "db2"), runs[0], ref):
                        assert got.dtype == (dtype if name in ("dx", "dh") else torch.float32), (what, name, got.dtype)
                        _check(got, want, f"{what} {name}")
                    if mode == "empty_row":
                        torch.testing.assert_close(runs[0][1][0], torch.full((T, G), 1.0 / T, device=DEV), rtol=1e-6, atol=0)


@pytest.mark.parametrize("x_dtype,h_dtype", [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32),
                                             (torch.float32, torch.float32)], ids=["x32_h16", "x16_h32", "x32_h32"])
def test_attflat_pool_pitched_rows_and_mixed_operands(x_dtype, h_dtype):
    """x as a column slice of a wider tensor (row pitch D + 8 > D, read in place: no copy) and the operand pair of the
    autocast step (fp32 encoder output, bf16 hidden activations) at the kernel bounds."""
    from sceneverse_amd.modules.heads import fused_attflat
    g = torch.Generator().manual_seed(77)
    for B, T, G, D, M in ((3, 65, 2, 768, 256), (2, 7, 1, 64, 8)):
        wide = torch.randn(B, T, D + 8, generator=g).to(DEV, x_dtype)
        x = wide[:, :, :D]
        assert fused_attflat._rows(x) is x and x.stride(1) == D + 8
        h = torch.randn(B, T, M, generator=g).to(DEV, h_dtype)
        w2 = (torch.randn(G, M, generator=g) / M ** 0.5).to(DEV)
        b2 = (0.1 * torch.randn(G, generator=g)).to(DEV)
        keep = (torch.rand(B, T, generator=g) > 0.4).to(DEV)
        keep[:, 0] = True
        dpooled = torch.randn(B, G * D, generator=g).to(DEV)
        ws_, hs, ww, bs = (t.detach().requires_grad_(True) for t in (wide, h, w2, b2))
        pooled, att = fused_attflat.attflat_pool(ws_[:, :, :D], hs, ww, bs, keep, return_att=True)
        pooled.backward(dpooled)
        ref = _attflat_ref(x, h, w2, b2, keep, dpooled)
        what = f"pitched B={B} T={T} G={G} D={D} M={M} x={x_dtype} h={h_dtype}"
        assert float(ws_.grad[:, :, D:].abs().max()) == 0.0, what          # nothing lands in the pad columns
        got = (pooled.detach(), att, ws_.grad[:, :, :D], hs.grad, ww.grad, bs.grad)
        assert got[2].dtype == x_dtype and got[3].dtype == h_dtype
        for name, a, b in zip(("pooled", "att", "dx", "dh", "dw2", "db2"), got, ref):
            _check(a, b, f"{what} {name}")


def test_attflat_shapes_outside_the_documented_ones_are_refused():
    from sceneverse_amd import _native
    lib = _native.load()
    x = torch.zeros(2, 513, 2056, device=DEV)
    h = torch.zeros(2, 513, 8, device=DEV)
    w = torch.zeros(5, 8, device=DEV)
    out = torch.zeros(2 * 5 * 2056 + 2 * 513 * 5, device=DEV)

    def fwd(B, T, G, D):
        return lib.gps_attflat_forward(B, T, G, D, 8, 0, x.data_ptr(), D, 0, h.data_ptr(), w.data_ptr(), w.data_ptr(), None,
                                       out.data_ptr(), out.data_ptr(), None)

    assert fwd(2, 513, 1, 64) == _native.GPS_ERR_UNSUPPORTED
    assert fwd(2, 7, 5, 64) == _native.GPS_ERR_UNSUPPORTED
    assert fwd(2, 7, 1, 2056) == _native.GPS_ERR_UNSUPPORTED
    assert fwd(0, 7, 1, 64) == _native.GPS_OK
    assert fwd(2, 7, 1, 64) == _native.GPS_OK
    torch.cuda.synchronize()


# ---- 1b: summed BCE with logits --------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 8), (3, 706), (2, 8864)])
def test_bce_logits_matches_fp64(rows, cols):
    from sceneverse_amd.optim.loss.fused_bce import bce_logits_sum, bce_logits_usable
    g = torch.Generator().manual_seed(17 * rows + cols)
    for x_dtype in (torch.bfloat16, torch.float32):
        for y_dtype in (torch.int64, torch.float32):
            for weighted in (False, True):
                x = 3 * torch.randn(rows, cols, generator=g)
                x.view(-1)[:4] = torch.tensor([80.0, -80.0, 80.0, -80.0])          # stability: both signs, both targets
                y = (torch.rand(rows, cols, generator=g) < 0.3).long()
                y.view(-1)[:4] = torch.tensor([0, 1, 1, 0])
                w = (torch.rand(rows, cols, generator=g) < 0.7) if weighted else None
                x, y = x.to(DEV, x_dtype), y.to(DEV, y_dtype)
                w = None if w is None else w.to(DEV)
                scale, gout = 1.0 / rows, torch.tensor(0.75, device=DEV)
                what = f"rows={rows} cols={cols} x={x_dtype} y={y_dtype} weighted={weighted}"
                assert bce_logits_usable(x, y, w), what
                runs = []
                for _ in range(2):
                    xs = x.clone().requires_grad_(True)
                    loss = bce_logits_sum(xs, y, w, scale)
                    loss.backward(gout)
                    runs.append((loss.detach(), xs.grad))
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), what
                x64 = x.double().requires_grad_(True)
                ref = F.binary_cross_entropy_with_logits(x64, y.double(), weight=None if w is None else w.double(),
                                                         reduction="sum") * scale
                ref.backward(gout.double())
                assert runs[0][0].dtype == torch.float32 and runs[0][1].dtype == x_dtype
                _check(runs[0][0], ref, what + " loss")
                _check(runs[0][1], x64.grad, what + " dx")


@pytest.mark.parametrize("cols,pitch", [(8864, 8872), (706, 712), (706, 707)])
def test_bce_logits_pitched_rows(cols, pitch):
    """Logits as a column slice of a wider tensor (row pitch > cols), read and differentiated in place; pitch 707 takes
    the element-access path."""
    from sceneverse_amd.optim.loss.fused_bce import bce_logits_sum
    g = torch.Generator().manual_seed(cols + pitch)
    for x_dtype in (torch.bfloat16, torch.float32):
        wide = (3 * torch.randn(3, pitch, generator=g)).to(DEV, x_dtype).requires_grad_(True)
        y = (torch.rand(3, cols, generator=g) < 0.3).long().to(DEV)
        w = (torch.rand(3, cols, generator=g) < 0.7).to(DEV)
        loss = bce_logits_sum(wide[:, :cols], y, w, 1.0 / 3)
        loss.backward()
        x64 = wide.detach()[:, :cols].double().requires_grad_(True)
        ref = F.binary_cross_entropy_with_logits(x64, y.double(), weight=w.double(), reduction="sum") / 3
        ref.backward()
        what = f"cols={cols} pitch={pitch} x={x_dtype}"
        assert float(wide.grad[:, cols:].abs().max()) == 0.0, what
        _check(loss.detach(), ref, what + " loss")
        _check(wide.grad[:, :cols], x64.grad, what + " dx")


# ---- 1c: TextObjWithinBatch, BCE branch ------------------------------------------------------------------------------
@pytest.mark.parametrize("B,O", [(1, 1), (1, 6), (3, 1), (3, 6), (3, 80), (1, 80)])
def test_text_obj_bce_matches_the_torch_branch_in_fp64(B, O):
    from sceneverse_amd.common.config import ConfigNode
    from sceneverse_amd.optim.loss import contra_loss
    from sceneverse_amd.optim.loss.fused_bce import text_obj_bce_usable
    g = torch.Generator().manual_seed(100 * B + O)
    D = 768
    obj, txt = torch.randn(B, O, D, generator=g), torch.randn(B, D, generator=g)
    masks = torch.rand(B, O, generator=g) > 0.3
    masks[:, 0] = True
    labels = (torch.rand(B, O, generator=g) < 0.3).long() * masks.long()
    if B > 1:
        masks[1] = False                                  # a fully padded scene
        labels[2] = 0                                     # an all-zero label row
    mod = contra_loss.TextObjWithinBatch(ConfigNode({"num_gpu": 1, "task": "ScanQA"}))

    def run(obj, txt):
        obj, txt = obj.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        loss = mod({"intra_obj_embeds": obj, "intra_text_embed": txt, "tgt_object_id": labels.to(obj.device),
                    "obj_masks": masks.to(obj.device)})
        loss.backward()
        return loss.detach(), obj.grad, txt.grad

    assert text_obj_bce_usable(obj.to(DEV), txt.to(DEV), labels.to(DEV), masks.to(DEV))
    got = run(obj.to(DEV), txt.to(DEV))
    again = run(obj.to(DEV), txt.to(DEV))
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    o64, t64 = obj.double().requires_grad_(True), txt.double().requires_grad_(True)      # the torch branch in fp64
    logits = torch.einsum("bod,bd->bo", F.normalize(o64, dim=-1, p=2), F.normalize(t64, dim=-1, p=2))
    ref = F.binary_cross_entropy_with_logits(logits, labels.double(), reduction="sum", weight=masks.double()) / float(B)
    ref.backward()
    want = (ref.detach(), o64.grad, t64.grad)
    for name, a, b in zip(("loss", "dobj", "dtext"), got, want):
        _check(a.cpu(), b, f"B={B} O={O} {name}")
    if O == 1:
        return                    # the torch branch squeezes a (B, 1) label matrix to (B,) and raises, like the reference's
    old = contra_loss._FUSED                              # the switch covers this branch: same value on the torch path
    contra_loss._FUSED = False
    try:
        torch.testing.assert_close(run(obj.to(DEV), txt.to(DEV))[0], got[0], rtol=1e-5, atol=1e-5)
    finally:
        contra_loss._FUSED = old


# ---- head, losses, model against the reference ---------------------------------------------------------------------
class _hip_only:
    """QA backend 'hip': a pooling call the library does not serve raises, so no torch fallback can hide."""

    def __enter__(self):
        from sceneverse_amd.modules.heads import qa_head
        qa_head.set_qa_backend("hip")

    def __exit__(self, *exc):
        from sceneverse_amd.modules.heads import qa_head
        qa_head.set_qa_backend("auto")
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


_HEAD_OPS = {"attflat_forward", "attflat_backward", "bce_logits_forward", "bce_logits_backward"}


@pytest.mark.parametrize("name", sorted(HEAD_CONFIGS))
def test_qa_head_gpu_fp32_matches_reference(gold, name):
    run_head(DEV, gold, name, 2e-3, FP32_GPU_GRADS)
    with _hip_only():
        ops = _count_native(lambda: run_head(DEV, gold, name, 2e-3, FP32_GPU_GRADS))
    assert _HEAD_OPS <= ops, ops


@pytest.mark.parametrize("name", sorted(HEAD_CONFIGS))
def test_qa_head_gpu_bf16_matches_reference(gold, name):
    run_head(DEV, gold, name, 6e-2, BF16_STEP_GRADS, autocast=True, ltol=3e-2)
    with _hip_only():
        ops = _count_native(lambda: run_head(DEV, gold, name, 6e-2, BF16_STEP_GRADS, autocast=True, ltol=3e-2))
    assert _HEAD_OPS | {"add_dropout_layernorm_forward", "add_dropout_layernorm_backward"} <= ops, ops
    assert any(k.startswith("gemm") for k in ops), ops              # the Linears ran on the library's GEMMs


def test_qa_model_gpu_fp32_matches_reference(gold):
    run_model(DEV, gold, 2e-3, FP32_GPU_GRADS)
    with _hip_only():
        ops = _count_native(lambda: run_model(DEV, gold, 2e-3, FP32_GPU_GRADS))
    assert _HEAD_OPS | {"text_obj_bce_forward", "text_obj_bce_backward"} <= ops, ops


def test_qa_model_gpu_bf16_matches_reference(gold):
    run_model(DEV, gold, 6e-2, BF16_STEP_GRADS, autocast=True, ltol=3e-2)
    with _hip_only():
        ops = _count_native(lambda: run_model(DEV, gold, 6e-2, BF16_STEP_GRADS, autocast=True, ltol=3e-2))
    assert _HEAD_OPS | {"text_obj_bce_forward", "text_obj_bce_backward"} <= ops, ops


def test_hip_backend_raises_on_a_call_the_library_does_not_serve():
    from sceneverse_amd.modules.heads.qa_head import AttFlat
    af = AttFlat(64, 16, 5, 32, 0.0).to(DEV).eval()       # 5 glimpses: outside the served shapes
    x = torch.randn(2, 7, 64, device=DEV)
    assert af(x, None).shape == (2, 32)                   # "auto": the torch composition
    with _hip_only(), pytest.raises(RuntimeError, match="unsupported"):
        af(x, None)


def test_qa_metrics_on_device_tensors(gold):
    from sceneverse_amd.engine import scanqa_accuracy, sqa3d_accuracy
    from tests.qa_cases import metric_inputs
    m = {k: v.to(DEV) for k, v in metric_inputs().items()}
    assert scanqa_accuracy(m["answer_scores"], m["answer_label"]) == gold["metrics_scanqa"]
    got = sqa3d_accuracy(m["answer_scores"], m["answer_label"], m["sqa_type"])
    assert all(got[k] == v for k, v in gold["metrics_sqa3d"].items() if k != "obj_cls_raw_acc")


# ---- the ScanQA train step: eager vs HIP graph -----------------------------------------------------------------------
def test_qa_train_step_graph_matches_eager_and_learns():
    """GPSTrainStep on the ScanQA-shaped config (QAHeadV1 with 8864 answers, answer_loss + BCE TextObjWithinBatch), 4
    scenes x 16 objects, 5 steps on one batch, dropout zeroed so both runs are deterministic functions of the weights:
    the captured step gives the eager losses within 2e-3 relative, `_graph` is set, the loss falls."""
    from bench import _lang_dir, gps_pretrain_cfg
    from sceneverse_amd.data.synthetic import synth_qa_batch
    from sceneverse_amd.engine import GPSTrainStep
    from sceneverse_amd.modules.layers.transformers import MultiheadSelfAttention

    def make(graph):
        cfg = as_qa_cfg(gps_pretrain_cfg(_lang_dir()))
        cfg.solver.sched.args.warmup_steps = 4
        st = GPSTrainStep(cfg, device=DEV, ddp=False, graph=graph, graph_warmup=2, seed=7)
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

    batch = synth_qa_batch(4, n_obj=16, seed=23, min_real=5, device=DEV)
    runs = {}
    for graph in (False, True):
        st = make(graph)
        losses = []
        for _ in range(5):
            total, parts = st.step(dict(batch))
            losses.append(total.item())
        assert set(parts) >= {"answer_loss", "TextObjWithinBatch", "total_loss"}
        if graph:
            assert st._graph is not None                  # steps 3.. were graph replays
        runs[graph] = losses
    eager, graphed = runs[False], runs[True]
    assert all(x == x for x in eager + graphed), runs
    for a, b in zip(eager, graphed):
        assert abs(a - b) <= 2e-3 * abs(a), runs
    assert eager[-1] < eager[0] and graphed[-1] < graphed[0], runs
