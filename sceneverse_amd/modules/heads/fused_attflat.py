"""The core of AttFlat on libgps_hip.so (csrc/gps_qa.hip): glimpse logits, masked softmax over the tokens and the
weighted pooling in one launch, their backward in two.

Reference: modules/heads/qa_head.py:56-67 after the first Linear + GELU (mlp.linear, masked_fill(-1e9), softmax(dim=1),
the per-glimpse weighted sums, cat).  GPU tensors, bf16 or fp32; anything else keeps the torch composition in qa_head.py."""
from __future__ import annotations

from typing import Optional

import torch

from ... import _native
from ..._launch import launch

MAX_T, MAX_G, MAX_D, MAX_M = 512, 4, 2048, 1024


def _rows(x: torch.Tensor) -> torch.Tensor:
    """x (B, T, D) with unit column stride and row (b, t) at (b T + t) pitch, copied when it is laid out otherwise."""
    B, T, D = x.shape
    ok = x.stride(2) == 1 and x.stride(1) % 8 == 0 and x.stride(1) >= D and (B == 1 or x.stride(0) == T * x.stride(1)) \
        and x.data_ptr() % 16 == 0
    return x if ok else x.contiguous()


def attflat_pool_usable(x: torch.Tensor, h: torch.Tensor, w2: torch.Tensor, keep: Optional[torch.Tensor] = None) -> bool:
    if not (x.is_cuda and h.is_cuda and w2.is_cuda and x.dim() == 3 and h.dim() == 3 and w2.dim() == 2):
        return False
    B, T, D = x.shape
    G, M = w2.shape
    return (x.dtype in (torch.bfloat16, torch.float32) and h.dtype in (torch.bfloat16, torch.float32)
            and h.shape == (B, T, M) and 0 < B <= 65535 and 1 <= T <= MAX_T and 1 <= G <= MAX_G
            and D % 8 == 0 and M % 8 == 0 and 0 < D <= MAX_D and 0 < M <= MAX_M
            and (keep is None or (keep.is_cuda and keep.shape == (B, T))))


class _AttFlatPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h, w2, b2, keep):
        B, T, D = x.shape
        G, M = w2.shape
        xr, hc = _rows(x), h.contiguous()
        w32, b32 = w2.detach().float().contiguous(), b2.detach().float().contiguous()
        keep8 = None
        if keep is not None:                   # bool masks are read in place, integer / float 0-1 masks cost one cast
            keep8 = (keep.view(torch.uint8) if keep.dtype == torch.bool else keep.to(torch.uint8)).contiguous()
        dev = x.device
        pooled = torch.empty((B, G * D), dtype=torch.float32, device=dev)
        att = torch.empty((B, T, G), dtype=torch.float32, device=dev)
        nbytes = xr.numel() * xr.element_size() + hc.numel() * hc.element_size() + 4 * (pooled.numel() + att.numel())
        launch("gps_attflat_forward", B, T, G, D, M, int(xr.dtype == torch.bfloat16), xr, xr.stride(1),
               int(hc.dtype == torch.bfloat16), hc, w32, b32, keep8, pooled, att, device=dev,
               label=f"attflat_forward(B={B},T={T},G={G},D={D},M={M})", nbytes=nbytes, what="attflat_forward")
        ctx.save_for_backward(xr, hc, w32, att, *(() if keep8 is None else (keep8,)))
        ctx.meta = (w2.dtype, b2.dtype)
        ctx.mark_non_differentiable(att)
        return pooled, att

    @staticmethod
    def backward(ctx, dpooled, _datt):
        xr, hc, w32, att, *rest = ctx.saved_tensors
        keep8 = rest[0] if rest else None
        B, T, D = xr.shape
        G, M = w32.shape
        dev = xr.device
        dpooled = dpooled.float().contiguous()
        dx = torch.empty((B, T, D), dtype=xr.dtype, device=dev) if ctx.needs_input_grad[0] else None
        dh = torch.empty_like(hc) if ctx.needs_input_grad[1] else None
        dw2 = torch.empty((G, M), dtype=torch.float32, device=dev)
        db2 = torch.empty(G, dtype=torch.float32, device=dev)
        ws = torch.empty(int(_native.load().gps_attflat_backward_ws_floats(B, T, G, M)), dtype=torch.float32, device=dev)
        nbytes = (xr.numel() * xr.element_size() * (2 if dx is not None else 1)
                  + hc.numel() * hc.element_size() * (2 if dh is not None else 1) + 4 * ws.numel())
        launch("gps_attflat_backward", B, T, G, D, M, int(xr.dtype == torch.bfloat16), xr, xr.stride(1),
               int(hc.dtype == torch.bfloat16), hc, w32, keep8, att, dpooled, dx, D, dh, dw2, db2, ws,
               _native.ticket(dev, "attflat"), device=dev, label=f"attflat_backward(B={B},T={T},G={G},D={D},M={M})",
               nbytes=nbytes, what="attflat_backward")
        w_dtype, b_dtype = ctx.meta
        return (dx, dh, dw2.to(w_dtype) if ctx.needs_input_grad[2] else None,
                db2.to(b_dtype) if ctx.needs_input_grad[3] else None, None)


def attflat_pool(x: torch.Tensor, h: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
                 keep: Optional[torch.Tensor] = None, return_att: bool = False):
    """x (B, T, D), h (B, T, M), w2 (G, M), b2 (G), keep (B, T) bool or 0 / 1 values, nonzero = valid token (None = all valid) ->
    pooled (B, G D) fp32 [, att (B, T, G) fp32, no gradient]."""
    pooled, att = _AttFlatPool.apply(x, h, w2, b2, keep)
    return (pooled, att.detach()) if return_att else pooled
