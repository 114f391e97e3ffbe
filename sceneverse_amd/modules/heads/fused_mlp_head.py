"""`get_mlp_head` stacks (modules/utils.py: Linear -> ReLU -> LayerNorm(eps 1e-12) -> Dropout -> Linear) on
libgps_hip.so (csrc/gps_ground.hip): everything behind the first Linear in one launch per direction.

Reference: modules/heads/grounding_head.py:20-27 -- `og3d_head(obj).squeeze(2)` + `masked_fill_(~obj_masks, -inf)`
-> `mlp_head_logit`; the hidden part of the three 607-class heads -> `mlp_head_hidden` (their last Linear stays torch's:
607 outputs are not a multiple of 8).  Either is ONE autograd node: under bf16 execution (`gemm.usable`) the first Linear
is the in-tree GEMM with its bias + ReLU epilogue on the bf16 shadow of the weight, backward = the tail kernel + the plain
input- and weight-gradient GEMMs; fp32 GPU tensors without autocast run torch's Linear and the same tail kernel in fp32
(`mlp_head_logit` only: the hidden output is bf16 by construction).  `seq[3].p` and `training` are read at call time.
GPU tensors only; the callers keep the torch composition for anything else."""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from ... import _native
from ..._launch import launch

MIN_D, MAX_D = 8, 1024


def _stack(seq):
    """(lin1, ln, drop, lin2) of a `get_mlp_head` Sequential, or None for anything else."""
    if not (isinstance(seq, nn.Sequential) and len(seq) == 5):
        return None
    lin1, act, ln, drop, lin2 = seq
    if not (isinstance(lin1, nn.Linear) and isinstance(act, nn.ReLU) and isinstance(ln, nn.LayerNorm)
            and isinstance(drop, nn.Dropout) and isinstance(lin2, nn.Linear)):
        return None
    d = lin1.out_features
    if (lin1.bias is None or lin2.bias is None or ln.weight is None or ln.bias is None
            or tuple(ln.normalized_shape) != (d,) or lin2.in_features != d):
        return None
    return lin1, ln, drop, lin2


def mlp_head_usable(x: torch.Tensor, seq) -> bool:
    """`seq` is the 5-element `get_mlp_head` Sequential, x and the parameters are on the GPU and the hidden width is one
    the tail kernels serve (a multiple of 8 in 8 .. 1024)."""
    st = _stack(seq)
    if st is None or not x.is_cuda or x.dim() < 2 or x.dtype not in (torch.bfloat16, torch.float32):
        return False
    lin1, ln, _, lin2 = st
    d = lin1.out_features
    return (x.shape[-1] == lin1.in_features and d % 8 == 0 and MIN_D <= d <= MAX_D and x.numel() > 0
            and all(p.is_cuda and p.dtype == torch.float32 for p in (lin1.weight, lin1.bias, ln.weight, ln.bias,
                                                                    lin2.weight, lin2.bias)))


def mlp_head_hidden_usable(x: torch.Tensor, seq) -> bool:
    """The hidden part is produced in bf16 for a following Linear: served under bf16 execution only."""
    from ..layers import gemm
    return mlp_head_usable(x, seq) and gemm.usable(x, seq[0].in_features, seq[0].out_features)


def _rows_view(h: torch.Tensor) -> torch.Tensor:
    """(n_rows, d) with unit column stride, a row pitch that is a multiple of 8 and a 16-byte aligned base; copied otherwise."""
    ok = h.dim() == 2 and h.stride(1) == 1 and h.stride(0) % 8 == 0 and h.stride(0) >= h.shape[1] and h.data_ptr() % 16 == 0
    return h if ok else h.contiguous()


def _vec16(t: torch.Tensor) -> torch.Tensor:
    """A parameter as a flat contiguous vector at a 16-byte aligned address (its own storage unless it is a view)."""
    v = t.detach().reshape(-1).contiguous()
    return v if v.data_ptr() % 16 == 0 else v.clone()


def _seed_args(p, seed, seed_dev):
    return float(p), int(seed) & ((1 << 64) - 1), seed_dev


def tail_forward(h: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, p: float = 0.0, seed: int = 0,
                 seed_dev: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None,
                 b2: Optional[torch.Tensor] = None, keep8: Optional[torch.Tensor] = None, want_z16: bool = False):
    """One launch of `gps_mlp_tail_forward`.  h (n_rows, d) bf16 / fp32 (a pitched view is read in place); gamma, beta (d)
    fp32; w2 (d), b2 (1) fp32 -> logit, else None; keep8 (n_rows) uint8.  -> (z16 or None, logit or None, mean, rstd)."""
    h = _rows_view(h)
    n, d = h.shape
    dev = h.device
    z16 = torch.empty((n, d), dtype=torch.bfloat16, device=dev) if want_z16 else None
    logit = torch.empty(n, dtype=torch.float32, device=dev) if w2 is not None else None
    mean = torch.empty(n, dtype=torch.float32, device=dev)
    rstd = torch.empty(n, dtype=torch.float32, device=dev)
    launch("gps_mlp_tail_forward", n, d, int(h.dtype == torch.bfloat16), h, h.stride(0), gamma, beta, float(eps),
           *_seed_args(p, seed, seed_dev), w2, b2, keep8, z16, logit, mean, rstd, device=dev,
           label=f"mlp_tail_forward(rows={n},d={d})", nbytes=n * d * (h.element_size() + (2 if want_z16 else 0)) + 12 * n,
           what="mlp_tail_forward")
    return z16, logit, mean, rstd


def tail_backward(h: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                  p: float = 0.0, seed: int = 0, seed_dev: Optional[torch.Tensor] = None,
                  w2: Optional[torch.Tensor] = None, keep8: Optional[torch.Tensor] = None,
                  dlogit: Optional[torch.Tensor] = None, dz16: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None):
    """One launch of `gps_mlp_tail_backward`.  dlogit (n_rows) fp32 and / or dz16 (n_rows, d) bf16; out: where dpre goes
    (h's dtype, may be a pitched view; default a new contiguous tensor).  -> (dpre, dgamma, dbeta, dw2, db2), all of the
    last four fp32; dw2 / db2 are None without dlogit."""
    h = _rows_view(h)
    n, d = h.shape
    dev = h.device
    dpre = torch.empty((n, d), dtype=h.dtype, device=dev) if out is None else out
    f = dict(dtype=torch.float32, device=dev)
    dgamma, dbeta = torch.empty(d, **f), torch.empty(d, **f)
    dw2 = torch.empty(d, **f) if dlogit is not None else None
    db2 = torch.empty(1, **f) if dlogit is not None else None
    partial = torch.empty(int(_native.load().gps_mlp_tail_partial_rows(n)) * (3 * d + 4), **f)
    nbytes = n * d * (2 * h.element_size() + (2 if dz16 is not None else 0)) + 12 * n + 4 * partial.numel()
    launch("gps_mlp_tail_backward", n, d, int(h.dtype == torch.bfloat16), h, h.stride(0), gamma, beta, mean, rstd,
           *_seed_args(p, seed, seed_dev), w2, keep8, dlogit, dz16, dpre, dpre.stride(0), dgamma, dbeta, dw2, db2, partial,
           _native.ticket(dev, "mlp_tail"), device=dev, label=f"mlp_tail_backward(rows={n},d={d})", nbytes=nbytes,
           what="mlp_tail_backward")
    return dpre, dgamma, dbeta, dw2, db2


class _MLPHeadFn(torch.autograd.Function):
    """x -> first Linear (+ ReLU) -> tail.  logit mode: fp32 (rows,) logits, -inf where keep == 0; hidden mode: the bf16
    (rows, d) input of the stack's last Linear."""

    @staticmethod
    def forward(ctx, x, w1, b1, gamma, beta, w2, b2, keep, eps, p, seed_dev, hidden):
        from ..layers import gemm
        bf16 = gemm.usable(x, w1.shape[1], w1.shape[0])
        if bf16:
            w16, b32 = gemm.shadow_of((w1,), (b1,))
            xr = gemm._as_rows16(x)
            h = gemm.linear_forward(xr, w16, b32, act="relu")
        else:
            w16 = None
            xr = x.reshape(-1, x.shape[-1])
            h = F.linear(xr, w1.detach(), b1.detach())              # pre-activation: the tail applies the ReLU
        g32, bt32 = _vec16(gamma), _vec16(beta)
        w2v = None if hidden else _vec16(w2)
        b2v = None if hidden else b2.detach().reshape(1)
        keep8 = None
        if keep is not None and not hidden:      # bool masks are read in place, integer / float 0-1 masks cost one cast
            keep8 = (keep.view(torch.uint8) if keep.dtype == torch.bool else keep.to(torch.uint8)).reshape(-1).contiguous()
        z16, logit, mean, rstd = tail_forward(h, g32, bt32, eps, p, 0, seed_dev, w2v, b2v, keep8, want_z16=hidden)
        saved = [xr, h, mean, rstd, g32, bt32]
        ctx.layout = (len(saved), w16 is not None, w2v is not None, keep8 is not None, seed_dev is not None)
        for t in (w16, w2v, keep8, seed_dev):
            if t is not None:
                saved.append(t)
        ctx.save_for_backward(*saved)
        ctx.meta = (x.shape, x.dtype, float(p), bool(hidden))
        ctx.params = (w1, b1)
        lead = x.shape[:-1]
        return z16.view(*lead, z16.shape[1]) if hidden else logit.view(*lead)

    @staticmethod
    def backward(ctx, dy):
        from ..layers import gemm
        n_fixed, has_w16, has_w2, has_keep, has_seed = ctx.layout
        saved = list(ctx.saved_tensors)
        xr, h, mean, rstd, g32, bt32 = saved[:n_fixed]
        rest = saved[n_fixed:]
        w16 = rest.pop(0) if has_w16 else None
        w2v = rest.pop(0) if has_w2 else None
        keep8 = rest.pop(0) if has_keep else None
        seed_dev = rest.pop(0) if has_seed else None
        x_shape, x_dtype, p, hidden = ctx.meta
        w1, b1 = ctx.params
        if hidden:
            dz16 = dy.reshape(-1, dy.shape[-1])
            dz16 = (dz16 if dz16.dtype == torch.bfloat16 else dz16.to(torch.bfloat16)).contiguous()
            dlogit = None
        else:
            dz16, dlogit = None, dy.reshape(-1).float().contiguous()
        dpre, dgamma, dbeta, dw2, db2 = tail_backward(h, g32, bt32, mean, rstd, p, 0, seed_dev, w2v, keep8, dlogit, dz16)
        need = ctx.needs_input_grad
        dx = dw1 = db1 = None
        if w16 is not None:
            if not (need[1] and need[2] and gemm._wgrad_to_params(dpre, xr, (w1,), (b1,), (w1.shape[0],))):
                if need[1] or need[2]:
                    dw1, db1 = gemm.linear_wgrad(dpre, xr, want_bias=True)
            if need[0]:
                dx = gemm._dx_out(gemm.linear_dgrad(dpre, w16), x_shape, x_dtype)
        else:
            if need[1]:
                dw1 = dpre.t().mm(xr.to(dpre.dtype)).to(w1.dtype)
            if need[2]:
                db1 = dpre.sum(0).to(b1.dtype)
            if need[0]:
                dx = dpre.mm(w1.detach().to(dpre.dtype)).to(x_dtype).view(x_shape)
        return (dx, dw1 if need[1] else None, db1 if need[2] else None,
                dgamma if need[3] else None, dbeta if need[4] else None,
                dw2.view(1, -1) if (dw2 is not None and need[5]) else None,
                db2 if (db2 is not None and need[6]) else None, None, None, None, None, None)


def _call(x, seq, keep, training, hidden):
    lin1, ln, drop, lin2 = _stack(seq)
    p = float(drop.p) if training else 0.0
    seed_dev = None
    if p > 0.0:
        from ..layers.fused_attention import _next_device_seed
        seed_dev = _next_device_seed(x.device)
    return _MLPHeadFn.apply(x, lin1.weight, lin1.bias, ln.weight, ln.bias, lin2.weight, lin2.bias, keep, float(ln.eps), p,
                            seed_dev, hidden)


def mlp_head_logit(x: torch.Tensor, seq, keep: Optional[torch.Tensor] = None, training: bool = False) -> torch.Tensor:
    """x (..., in) through a 1-output `get_mlp_head` stack -> fp32 (...,) logits, exactly -inf where keep (...,) is zero
    (bool or 0 / 1 values; None = nothing masked).  Masked rows pass no gradient."""
    return _call(x, seq, keep, training, False)


def mlp_head_hidden(x: torch.Tensor, seq, training: bool = False) -> torch.Tensor:
    """x (..., in) through `seq[0:4]` -> bf16 (..., hidden), the input of `seq[4]` (bf16 execution only)."""
    return _call(x, seq, None, training, True)
