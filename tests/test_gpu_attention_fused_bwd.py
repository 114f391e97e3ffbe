"""One-launch plain attention backward (gps_attention_fa.hip bwd_fused_kernel: a workgroup owns a whole (sequence,
head), every score / probability / dS element formed once, dQ accumulated in registers over the key blocks; plain-mode
bit 8) against the whole-sequence kernels of gps_attention.hip (mode 0) on the SAME inputs with the same dropout stream
and lse, in the pattern and at the tolerances of tests/test_gpu_attention_blocks.py: out <= 1e-2 max, each of dq / dk /
dv <= 1.5e-2 max of the whole gradient.  Mode 13 = 1 | 4 | 8 is the product default; fixed-length rows up to 144 tokens
would go to the K / V-resident kernels there (bit 4 goes first), so those lengths run mode 9 = 1 | 8."""
import functools

import pytest
import torch

from sceneverse_amd.modules.layers import fused_attention as FA

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 12
D = H * 64
FUSED = 1 | 4 | 8


def _close(a, b, tol, what):
    a, b = a.float(), b.float()
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= tol * ref + 1e-6, (what, err, ref)


def _in_mode(mode, run):
    FA.set_plain_mode(mode)
    try:
        return run()
    finally:
        FA.set_plain_mode()


def _grads_close(g_b, g_w, scale=None):
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        if scale is None:
            _close(g_b[..., sl], g_w[..., sl], 1.5e-2, name)
        else:
            err = (g_b[..., sl].float() - g_w[..., sl].float()).abs().max().item()
            assert err <= 1.5e-2 * scale + 1e-6, (name, err, scale)


@pytest.mark.parametrize("L", [1, 15, 16, 17, 63, 64, 65, 129, 130, 300, 320, 321])
@pytest.mark.parametrize("B", [3, 2])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_self_attention_with_mask_and_dropout(B, L, p):
    g = torch.Generator().manual_seed(B * 100 + L)
    packed = torch.randn(B, L, 3 * D, generator=g).to(torch.bfloat16).to(DEV)
    n_real = torch.randint(1, L + 1, (B,), generator=g)
    n_real[0] = L
    mask = (torch.arange(L)[None, :] >= n_real[:, None]).to(DEV)
    go = torch.randn(B, L, D, generator=g).to(torch.bfloat16).to(DEV)
    seed_dev = torch.tensor([12345], dtype=torch.int64, device=DEV)

    def run():
        x = packed.clone().requires_grad_(True)
        out = FA._FusedSelfAttention.apply(x, None, mask, H, p, 77, seed_dev if p else None)
        out.backward(go)
        return out.detach(), x.grad.detach()
    o_w, g_w = _in_mode(0, run)
    o_b, g_b = _in_mode(9 if L <= 144 else FUSED, run)       # L = 321: past the kernel's capacity, the fallback must agree
    valid = ~mask
    assert torch.isfinite(o_b[valid]).all() and torch.isfinite(g_b).all()
    _close(o_b[valid], o_w[valid], 1e-2, "out")
    # scale = the whole gradient tensor's (with one live key dq and dk are exactly 0 in exact arithmetic)
    _grads_close(g_b[valid], g_w[valid], g_w[valid].abs().max().item())
    if mask.any():
        assert g_b[..., D:][mask].abs().max().item() == 0.0      # padded keys: dk = dv = exact zeros


@functools.lru_cache(maxsize=None)
def _varlen_inputs():
    g = torch.Generator().manual_seed(3)
    lens = torch.cat([torch.randint(6, 51, (10,), generator=g), torch.randint(30, 301, (10,), generator=g),
                      torch.tensor([300, 1, 64, 65, 0])])
    n_seq = lens.numel()
    cu = torch.zeros(n_seq + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    T = int(cu[-1]) + 7                                       # rows behind the last sequence: never touched
    packed = torch.randn(T, 3 * D, generator=g).to(torch.bfloat16).to(DEV)
    go = torch.randn(T, D, generator=g).to(torch.bfloat16).to(DEV)
    order = torch.argsort(lens, descending=True).to(torch.int32).to(DEV)
    q_limit = lens.clone().to(torch.int32)
    q_limit[10:] = 1                                          # the long ones: read at their first row only (last BERT layer)
    seed_dev = torch.tensor([999], dtype=torch.int64, device=DEV)
    return lens, cu, T, packed, go, order, q_limit.to(DEV), cu.to(DEV), seed_dev


def _computed_rows(lens, cu, T, q_limit):
    rows = torch.zeros(T, dtype=torch.bool)
    for s in range(lens.numel()):
        n = int(lens[s]) if q_limit is None else min(int(lens[s]), int(q_limit[s]))
        rows[int(cu[s]):int(cu[s]) + n] = True
    return rows.to(DEV)


def _varlen_run(p, q_limit):
    lens, cu, T, packed, go, order, _, cu_d, seed_dev = _varlen_inputs()
    rows = _computed_rows(lens, cu, T, q_limit)
    x = packed.clone().requires_grad_(True)
    out = FA._FusedVarlenSelfAttention.apply(x, cu_d, lens.numel(), 300, H, p, seed_dev if p else None, order, q_limit)
    out = torch.where(rows[:, None], out, torch.zeros_like(out))      # rows that are not computed hold garbage
    return x, out, go, rows


@functools.lru_cache(maxsize=None)
def _varlen_whole(p, use_limit):
    """the whole-sequence result of one (p, limit) case: computed once, shared, never modified"""
    def run():
        x, out, go, _ = _varlen_run(p, _varlen_inputs()[6] if use_limit else None)
        (out.float() * go.float()).sum().backward()
        return out.detach(), x.grad.detach()
    return _in_mode(0, run)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("use_limit", [False, True])
def test_packed_variable_length_sequences(p, use_limit):
    lens, cu, T = _varlen_inputs()[:3]
    n_rows = int(cu[-1])

    def run():
        x, out, go, rows = _varlen_run(p, _varlen_inputs()[6] if use_limit else None)
        (out.float() * go.float()).sum().backward()
        return out.detach(), x.grad.detach(), rows
    o_w, g_w = _varlen_whole(p, use_limit)
    o_b, g_b, rows = _in_mode(FUSED, run)
    assert torch.isfinite(o_b).all() and torch.isfinite(g_b[:n_rows]).all()
    _close(o_b, o_w, 1e-2, "out")
    _grads_close(g_b[:n_rows], g_w[:n_rows])
    if use_limit:
        skipped = ~rows[:n_rows]
        assert skipped.any() and g_b[:n_rows, :D][skipped].abs().max().item() == 0.0     # dQ past the limit: exact zeros


def test_joint_form():
    lens = torch.tensor([130, 129, 78, 64, 17, 1])
    g = torch.Generator().manual_seed(130)
    cu = torch.zeros(lens.numel() + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    T = int(cu[-1])
    packed = torch.randn(T, 3 * D, generator=g).to(torch.bfloat16).to(DEV)
    go = torch.randn(T, D, generator=g).to(torch.bfloat16).to(DEV)
    cu_d = cu.to(DEV)
    seed_dev = torch.tensor([4242], dtype=torch.int64, device=DEV)

    def run():
        x = packed.clone().requires_grad_(True)
        out = FA._FusedVarlenSelfAttention.apply(x, cu_d, lens.numel(), 130, H, 0.1, seed_dev, None, None)
        out.backward(go)
        return out.detach(), x.grad.detach()
    o_w, g_w = _in_mode(0, run)
    o_b, g_b = _in_mode(FUSED, run)
    assert torch.isfinite(o_b).all() and torch.isfinite(g_b).all()
    _close(o_b, o_w, 1e-2, "out")
    _grads_close(g_b, g_w)


@pytest.mark.parametrize("use_limit", [False, True])
def test_backward_is_bit_reproducible(use_limit):
    n_rows = int(_varlen_inputs()[1][-1])

    def run():
        x, out, go, _ = _varlen_run(0.1, _varlen_inputs()[6] if use_limit else None)
        first, = torch.autograd.grad(out, x, go, retain_graph=True)
        second, = torch.autograd.grad(out, x, go)
        return first[:n_rows], second[:n_rows]
    first, second = _in_mode(FUSED, run)
    for name, sl in (("dq", slice(0, D)), ("dk", slice(D, 2 * D)), ("dv", slice(2 * D, 3 * D))):
        assert torch.equal(first[:, sl], second[:, sl]), name
