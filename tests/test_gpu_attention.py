"""Fused self-attention core (gps_attn_forward / gps_attn_backward, bf16 MFMA) against the fp32
torch formulation of the same math (the formulation tests/test_oracle_vs_golden.py pins to the
reference's modules/layers/transformers.py:193-239 and :141).

Both sides start from the SAME bf16-rounded q/k/v; the fused kernel additionally rounds the
probabilities and its outputs to bf16 (as the autocast torch path does).  Tolerances:
  forward   |diff| <= 2e-2 * max|ref|   (bf16 has 8 mantissa bits: 2^-8 = 3.9e-3 per rounding)
  backward  |diff| <= 4e-2 * max|ref| per gradient tensor
Edge cases: ragged lengths (L not a multiple of 16), padded keys, B not a multiple of 8 (no XCD
swizzle) and B = 8 (swizzled), no spatial term, dropout (adjoint + linearity identities)."""
import math

import pytest
import torch

from sceneverse_amd.modules.layers.fused_attention import _FusedSelfAttention
from sceneverse_amd.modules.layers import transformers as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 12
D = H * 64


def _inputs(B, L, spatial, seed=0, pad=True):
    g = torch.Generator().manual_seed(seed)
    W = 3 * D + (H * 6 if spatial else 0)
    packed = torch.randn(B, L, W, generator=g)
    if spatial:
        packed[..., 3 * D:] *= 2.0
    packed = packed.to(torch.bfloat16)
    pl = (torch.rand(B, L, L, 5, generator=g) * 2 - 1) if spatial else None
    mask = None
    if pad:
        n_real = torch.randint(max(1, L // 3), L + 1, (B,), generator=g)
        mask = torch.arange(L)[None, :] >= n_real[:, None]
    return packed, pl, mask


def ref_attention(packed, pl, mask):
    """fp32 reference; packed float32 (B,L,W) requires_grad."""
    B, L, W = packed.shape
    q, k, v = (packed[..., i * D:(i + 1) * D].view(B, L, H, 64).transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(64)
    if pl is not None:
        sw = packed[..., 3 * D:].view(B, L, H, 6).permute(0, 2, 1, 3)
        loc = torch.sigmoid(torch.einsum('bhld,bltd->bhlt', sw[..., 1:], pl) + sw[..., :1])
        if mask is not None:
            loc = loc.masked_fill(mask[:, None, None, :], 0)
        s = s + torch.log(torch.clamp(loc, min=1e-6))
    if mask is not None:
        s = s.masked_fill(mask[:, None, None, :], float('-inf'))
    p = torch.softmax(s, dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, L, D)


def _close(a, b, tol, what):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= tol * ref + 1e-6, (what, err, ref)


CASES = [(3, 80, True), (8, 80, True), (2, 130, False), (8, 130, False), (2, 37, True), (1, 200, True),
         (2, 16, False), (2, 256, False), (2, 300, False), (1, 300, True), (8, 300, False), (2, 512, False),
         (1, 145, True), (2, 177, False)]


@pytest.fixture(params=["default", "resident", "streaming", "planes", "blocks", "kv-resident", "fused-bwd", "product"])
def family(request):
    """Which kernels serve a call.  "product" is the plain form as the training step runs it (plain mode 13 = 1 | 4 | 8:
    K / V-resident kernels up to 144 tokens, above that the block-streaming forward with the one-launch backward of
    gps_attention_fa.hip up to 320 tokens and the whole-sequence backward beyond), "fused-bwd" (mode 9 = 1 | 8) that
    forward and the one-launch backward at every length up to 320.  The two PRODUCT defaults:
      "planes"  the spatial form on gps_attention_sp.hip (fp16 planes of the pairwise tensor, bf16 conditioning vector
                read in place; L <= 144),
      "blocks"  the plain form on the block-streaming kernels of gps_attention_fa.hip (any length; forward AND backward --
                the product takes their forward only where "kv-resident" does not apply),
      "kv-resident"  the plain form of fixed-length rows up to 144 tokens on the K / V-resident kernels of
                gps_attention_sp.hip.
    The other three run the GENERAL kernels of gps_attention.hip (interleaved fp32 pairwise tensor, whole-sequence
    workgroups): their own split (plain -> streaming, spatial -> register-resident), all register-resident, or all
    streaming (gps_attn_set_stream_min_tiles); rows above 144 tokens always stream there."""
    from sceneverse_amd import _native
    from sceneverse_amd.modules.layers import fused_attention as FA
    lib = _native.load()
    lib.gps_attn_set_stream_min_tiles(*{"resident": (10, 10), "streaming": (1, 1)}.get(request.param, (1, 10)))
    FA.set_spatial_planes(request.param == "planes")
    FA.set_plain_mode({"blocks": 3, "kv-resident": 4, "fused-bwd": 9, "product": 13}.get(request.param, 0))
    yield request.param
    lib.gps_attn_set_stream_min_tiles(1, 10)
    FA.set_spatial_planes(True)
    FA.set_plain_mode()


def _skip_duplicates(family, L, spatial):
    if family in ("resident", "streaming") and L > 144:
        pytest.skip("rows above 144 tokens stream in every setting of the general kernels")
    if family == "planes" and (not spatial or L > 144):
        pytest.skip("the plane form is the spatial term's, up to 144 tokens")
    if family in ("blocks", "fused-bwd", "product") and spatial:
        pytest.skip("the block-streaming kernels, the one-launch backward and the plain mode serve the plain form")
    if family == "kv-resident" and (spatial or L > 144):
        pytest.skip("the K / V-resident plain kernels serve fixed-length rows up to 144 tokens")


@pytest.mark.parametrize("B,L,spatial", CASES)
def test_forward_backward_match_fp32_formulation(B, L, spatial, family):
    _skip_duplicates(family, L, spatial)
    packed, pl, mask = _inputs(B, L, spatial, seed=B * 1000 + L)
    ref_in = packed.float().requires_grad_(True)
    ref = ref_attention(ref_in, pl, mask)
    go = torch.randn(B, L, D, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    ref.backward(go.float())

    x = packed.to(DEV).requires_grad_(True)
    out = _FusedSelfAttention.apply(x, pl.to(DEV) if pl is not None else None,
                                    mask.to(DEV) if mask is not None else None, H, 0.0, 0, None)
    out.backward(go.to(DEV))
    _close(out, ref, 2e-2, "out")
    g, gr = x.grad.float().cpu(), ref_in.grad

    def rel_l2(a, b):
        return ((a.float().cpu() - b).norm() / (b.norm() + 1e-20)).item()
    assert rel_l2(out, ref.detach()) <= 1e-2, ("out rel-L2", rel_l2(out, ref.detach()))
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        _close(g[..., sl], gr[..., sl], 4e-2, name)
        # relative L2 against the fp32 formulation: the bf16 rounding of the stored gradient is 2 - 3e-3
        assert rel_l2(g[..., sl], gr[..., sl]) <= 1e-2, (name, rel_l2(g[..., sl], gr[..., sl]))
    if spatial:
        _close(g[..., 3 * D:], gr[..., 3 * D:], 4e-2, "dsw")
    # padded keys receive no gradient through k and v
    if mask is not None and mask.any():
        assert g[..., D:3 * D][mask].abs().max().item() == 0.0


def test_streaming_and_resident_kernels_agree_at_the_switch():
    """L = 144 runs the register-resident kernels, L = 145 the streaming ones: same inputs (one padded token
    more) must give the same first 144 rows to bf16 rounding, with dropout active (one shared RNG stream)."""
    from sceneverse_amd import _native
    from sceneverse_amd.modules.layers import fused_attention as FA
    FA.set_plain_mode(0)                                      # the general kernels' own two families
    _native.load().gps_attn_set_stream_min_tiles(10, 10)      # the plain form streams from one tile on by default
    packed, _, _ = _inputs(2, 145, False, seed=31, pad=False)
    mask = torch.zeros(2, 145, dtype=torch.bool)
    mask[:, 144] = True                                       # the extra key is padding
    x145 = packed.to(DEV)
    x144 = packed[:, :144].contiguous().to(DEV)
    o145 = _FusedSelfAttention.apply(x145, None, mask.to(DEV), H, 0.0, 0, None)
    o144 = _FusedSelfAttention.apply(x144, None, None, H, 0.0, 0, None)
    _native.load().gps_attn_set_stream_min_tiles(1, 10)
    FA.set_plain_mode()
    _close(o145[:, :144], o144, 1e-2, "switch")


@pytest.mark.parametrize("L", [80, 200, 300])
def test_dropout_is_reproducible_linear_and_adjoint(L, family):
    if family in ("planes", "blocks", "kv-resident", "fused-bwd", "product"):
        pytest.skip("this test drives the SPATIAL form with dropout: served by the general kernels (other families)")
    _skip_duplicates(family, L, True)
    B = 2
    packed, pl, mask = _inputs(B, L, True, seed=9)
    pl, mask = pl.to(DEV), mask.to(DEV)
    p, seed = 0.3, 1234567

    def run(pk):
        return _FusedSelfAttention.apply(pk, pl, mask, H, p, seed, None)

    x = packed.to(DEV)
    o1, o2 = run(x), run(x)
    assert torch.equal(o1, o2)                                   # same seed -> same mask
    o3 = _FusedSelfAttention.apply(x, pl, mask, H, p, seed + 1, None)
    assert not torch.equal(o1, o3)
    o0 = _FusedSelfAttention.apply(x, pl, mask, H, 0.0, 0, None)
    # a device-side seed word is added to the host seed: (seed, dev=1) == (seed + 1, dev=None)
    dev1 = torch.tensor([1], dtype=torch.int64, device=DEV)
    assert torch.equal(_FusedSelfAttention.apply(x, pl, mask, H, p, seed, dev1), o3)
    # E[dropout(P)] = P: averaged over all outputs the two agree to a few percent
    assert abs(o1.float().mean().item() - o0.float().mean().item()) < 0.05 * o0.float().abs().mean().item() + 1e-3
    # adjoint identity in v (out is linear in v for a fixed keep mask): <out(v), g> == <v, dv>
    xg = x.clone().requires_grad_(True)
    out = run(xg)
    # a cotangent correlated with the output, so that neither inner product is a cancelling sum (bf16 rounding of
    # out and dv stays far below the tolerance while a wrong keep mask in the backward moves rhs by tens of percent)
    gen = torch.Generator(device=DEV).manual_seed(77)
    go = (out.detach().float() * (1.0 + 0.5 * torch.randn(B, L, D, device=DEV, generator=gen))).to(torch.bfloat16)
    out.backward(go)
    lhs = (out.float() * go.float()).sum().item()
    rhs = (xg.detach()[..., 2 * D:3 * D].float() * xg.grad[..., 2 * D:3 * D].float()).sum().item()
    assert abs(lhs - rhs) <= 2e-2 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_layers_hip_backend_matches_torch_backend_under_autocast():
    torch.manual_seed(0)
    B, L = 4, 80
    layer = T.TransformerSpatialEncoderLayer(768, 12, dim_feedforward=2048, dropout=0.0, activation="gelu",
                                             spatial_multihead=True, spatial_dim=5,
                                             spatial_attn_fusion='cond').to(DEV)
    joint = T.TransformerEncoderLayer(768, 12, dim_feedforward=2048, dropout=0.0).to(DEV)
    x = torch.randn(B, L, 768, device=DEV)
    pl = torch.rand(B, L, L, 5, device=DEV) * 2 - 1
    mask = torch.arange(L, device=DEV)[None, :] >= torch.tensor([80, 33, 50, 61], device=DEV)[:, None]
    res = {}
    for backend in ("hip", "torch"):
        T.set_attention_backend(backend)
        for m in (layer, joint):
            m.zero_grad(set_to_none=True)
        xin = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y, _ = layer(xin, pl, tgt_key_padding_mask=mask)
            z, _ = joint(y, tgt_key_padding_mask=mask)
        z.float().square().mean().backward()
        res[backend] = (z.detach().float(), xin.grad.detach().float(),
                        layer.self_attn.lang_cond_fc.weight.grad.detach().float(),
                        joint.self_attn.in_proj_weight.grad.detach().float())
    T.set_attention_backend("auto")
    names = ("output", "dx", "d lang_cond_fc.weight", "d in_proj_weight")
    for a, b, n in zip(res["hip"], res["torch"], names):
        _close(a, b, 5e-2, n)


def test_fp32_inputs_run_the_fp32_core_not_the_bf16_one():
    """fp32 tensors without autocast go to the fp32-operand kernels (fp32 MFMA): the result stays fp32 and agrees
    with the torch formulation to fp32 rounding, far below what a detour through bf16 would leave."""
    layer = T.TransformerEncoderLayer(768, 12, dropout=0.0).to(DEV).eval()
    x = torch.randn(2, 50, 768, device=DEV)
    from sceneverse_amd.pointnet2 import _ext
    _ext.profile_start()
    y, _ = layer(x)
    seen = _ext.profile_stop()
    assert y.dtype == torch.float32
    assert any(k.startswith("attn_forward") and k.endswith("[fp32]") for k in seen), sorted(seen)
    T.set_attention_backend("torch")
    try:
        want, _ = layer(x)
    finally:
        T.set_attention_backend("auto")
    _close(y, want, 1e-4, "fp32 layer")


def test_full_bench_shapes_against_reference_on_sampled_scenes():
    """BASELINE sizes: B = 64, spatial L = 80 and joint L = 130.  The fused kernel runs on the whole
    batch; two sampled scenes are recomputed with the fp32 formulation.  Batch elements are
    independent, so evaluating a sub-batch alone must reproduce its rows bit for bit."""
    for L, spatial in ((80, True), (130, False)):
        packed, pl, mask = _inputs(64, L, spatial, seed=L)
        x = packed.to(DEV)
        plg = pl.to(DEV) if pl is not None else None
        mg = mask.to(DEV)
        out = _FusedSelfAttention.apply(x, plg, mg, H, 0.0, 0, None)
        for b in (3, 41):
            ref = ref_attention(packed[b:b + 1].float(), pl[b:b + 1] if pl is not None else None, mask[b:b + 1])
            _close(out[b:b + 1], ref, 2e-2, f"L={L} scene {b}")
        sub = _FusedSelfAttention.apply(x[8:16].contiguous(), plg[8:16].contiguous() if plg is not None else None,
                                        mg[8:16].contiguous(), H, 0.0, 0, None)
        assert torch.equal(sub, out[8:16])


def _rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@pytest.mark.parametrize("L,spatial", [(80, True), (130, False), (37, True)])
def test_fused_core_against_the_pinned_oracle_formulation(L, spatial):
    """gps_attn_forward / gps_attn_backward against oracle/gps_torch_reference.py (the restatement that
    tests/test_oracle_vs_golden.py pins to the reference's own outputs), not against a test-local formula.
    The q / k / v / output projections are identities, so the oracle's fp32 module and the product's bf16 module
    see the same bf16-exact q = k = v = x and every difference comes from the attention core (+ the bf16
    rounding of the conditioning vector).  Bounds: relative L2 <= 1e-2 per tensor AND max-norm 4e-2."""
    from oracle import gps_torch_reference as R
    B = 3
    g = torch.Generator().manual_seed(1000 + L)
    x = torch.randn(B, L, D, generator=g).to(torch.bfloat16).float()
    n_real = torch.randint(max(2, L // 3), L + 1, (B,), generator=g)
    pad = torch.arange(L)[None, :] >= n_real[:, None]
    go = torch.randn(B, L, D, generator=g).to(torch.bfloat16).float()
    eye = torch.eye(D)
    if spatial:
        mod = T.MultiHeadAttentionSpatial(D, H, spatial_multihead=True, spatial_dim=5, spatial_attn_fusion='cond')
        with torch.no_grad():
            for lin in (mod.w_qs, mod.w_ks, mod.w_vs, mod.fc):
                lin.weight.copy_(eye)
                lin.bias.zero_()
            mod.lang_cond_fc.weight.copy_((0.05 * torch.randn(H * 6, D, generator=g)).to(torch.bfloat16).float())
            mod.lang_cond_fc.bias.copy_(0.1 * torch.randn(H * 6, generator=g))
        pl = torch.rand(B, L, L, 5, generator=g) * 2 - 1
        sd = {f"a.{k}": v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
        xr = x.clone().requires_grad_(True)
        ref, _ = R.spatial_attention(sd, "a", xr, pl, pad, H)
    else:
        mod = T.MultiheadSelfAttention(D, H, dropout=0.0)
        with torch.no_grad():
            mod.in_proj_weight.copy_(torch.cat([eye, eye, eye], 0))
            mod.in_proj_bias.zero_()
            mod.out_proj.weight.copy_(eye)
            mod.out_proj.bias.zero_()
        pl = None
        sd = {f"a.{k}": v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
        xr = x.clone().requires_grad_(True)
        ref, _ = R.mha_self_attention(sd, "a", xr, pad, H)
    ref.backward(go)

    mod = mod.to(DEV).eval()
    xg = x.to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        if spatial:
            out, _ = mod(xg, xg, xg, pl.to(DEV), key_padding_mask=pad.to(DEV))
        else:
            out, _ = mod(xg, xg, xg, key_padding_mask=pad.to(DEV))
    assert out.dtype == torch.bfloat16                      # went through the fused bf16 path
    out.backward(go.to(DEV).to(out.dtype))
    checks = [("out", out, ref), ("dx", xg.grad, xr.grad)]
    params = dict(mod.named_parameters())
    names = ["lang_cond_fc.weight", "lang_cond_fc.bias", "w_qs.weight", "w_ks.weight", "w_vs.weight", "fc.weight"] \
        if spatial else ["in_proj_weight", "in_proj_bias", "out_proj.weight"]
    for n in names:
        checks.append((f"d {n}", params[n].grad, sd[f"a.{n}"].grad))
    for what, a, b in checks:
        assert _rel_l2(a, b) <= 1e-2, (what, _rel_l2(a, b))
        _close(a, b, 4e-2, what)


# ---------------------------------------------------------------------------------------------------------------
# plane form of the spatial term (gps_attention_sp.hip) against the general kernels on the SAME inputs
# ---------------------------------------------------------------------------------------------------------------
def _run_spatial(packed, pl, mask, go, planes):
    from sceneverse_amd.modules.layers import fused_attention as FA
    FA.set_spatial_planes(planes)
    try:
        x = packed.clone().requires_grad_(True)
        out = _FusedSelfAttention.apply(x, pl, mask, H, 0.0, 0, None)
        out.backward(go)
        return out.detach().float(), x.grad.detach().float()
    finally:
        FA.set_spatial_planes(True)


@pytest.mark.parametrize("B,L", [(64, 80), (3, 80), (2, 16), (2, 17), (1, 1), (2, 50), (8, 81), (2, 144), (5, 100), (2, 79)])
@pytest.mark.parametrize("w_scale", [2.0, 40.0])
def test_plane_form_equals_the_general_kernels(B, L, w_scale):
    """Same bf16 q / k / v / conditioning vector, same key-padding mask.  Differences allowed: the pairwise features are
    rounded to fp16 (<= 2.5e-4 absolute on values in [-1, 1], against 4e-3 relative of the bf16 conditioning weights they
    multiply) and delta = rowsum(dO * O) from the bf16 forward output instead of rowsum(P dP) -- both below the bf16
    rounding of the results: |diff| <= 1.5e-2 max|ref| per tensor (w_scale 40 drives most pairs into the clamp
    log(1e-6) / the saturated sigmoid, where the gate of the spatial gradient must be exactly 0)."""
    g = torch.Generator().manual_seed(L * 31 + B)
    packed = torch.randn(B, L, 3 * D + 6 * H, generator=g)
    packed[..., 3 * D:] *= w_scale
    packed = packed.to(torch.bfloat16).to(DEV)
    pl = (torch.rand(B, L, L, 5, generator=g) * 2 - 1).to(DEV)
    n_real = torch.randint(1, L + 1, (B,), generator=g)
    n_real[0] = L
    mask = (torch.arange(L)[None, :] >= n_real[:, None]).to(DEV)
    go = torch.randn(B, L, D, generator=g).to(torch.bfloat16).to(DEV)
    o_ref, g_ref = _run_spatial(packed, pl, mask, go, planes=False)
    o_new, g_new = _run_spatial(packed, pl, mask, go, planes=True)
    assert torch.isfinite(o_new).all() and torch.isfinite(g_new).all()
    _close(o_new, o_ref, 1.5e-2, "out")
    scale = g_ref.abs().max().item()              # one key: dq / dk / dsw are 0 up to p (1 - p) ~ 1e-6 of the cotangent
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D)), ("dsw", slice(3 * D, None))):
        err = (g_new[..., sl] - g_ref[..., sl]).abs().max().item()
        assert err <= 1.5e-2 * g_ref[..., sl].abs().max().item() + 1e-5 * scale, (name, err)
    assert g_new[..., D:3 * D][mask].abs().max().item() == 0.0 if mask.any() else True


def test_pairwise_planes_are_the_fp16_image_of_the_pairwise_tensor():
    """gps_pairwise_locs_planes (the attribute calc_pairwise_locs attaches) and gps_pairwise_to_planes (tensors built
    elsewhere): planes[b][d][l][t] == fp16(pl[b][l][t][d]) exactly, pad columns zero."""
    from sceneverse_amd.modules.utils import calc_pairwise_locs, pairwise_planes
    for L in (80, 37, 6):
        centers = (torch.rand(3, L, 3, generator=torch.Generator().manual_seed(L)) * 8 - 4).to(DEV)
        pl = calc_pairwise_locs(centers, None)
        planes = pl._gps_planes
        ld = planes.shape[-1]
        assert planes.shape == (3, 5, L, ld) and ld % 4 == 0 and ld >= L
        want = pl.permute(0, 3, 1, 2).to(torch.float16)
        assert torch.equal(planes[..., :L], want) and (planes[..., L:] == 0).all()
        again = pairwise_planes(pl.clone())                      # no attribute on the clone: the conversion launch
        assert torch.equal(again, planes)
        ref = calc_pairwise_locs(centers.cpu(), None)            # the torch formulation
        assert (pl.cpu() - ref).abs().max().item() <= 1e-6
