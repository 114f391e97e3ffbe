"""og3d_loss on libgps_hip.so (csrc/gps_ground.hip `og3d_ce_kernel`): one launch writes the loss and its unit logit
gradient, the backward pass is one elementwise scale.

Reference: optim/loss/loss.py:8-9 -- F.cross_entropy(og3d_logits (B, O), tgt_object_id.squeeze(1)) with torch's defaults
(mean over the rows whose target is not -100); the logits hold -inf at the padded objects.  GPU tensors only; the caller
keeps F.cross_entropy for anything else."""
from __future__ import annotations

import torch

from ... import _native
from ..._launch import launch

MAX_O = 512


def og3d_ce_usable(logits: torch.Tensor, target: torch.Tensor) -> bool:
    return (logits.is_cuda and target.is_cuda and logits.dim() == 2 and logits.dtype in (torch.float32, torch.bfloat16)
            and target.dtype == torch.int64 and logits.shape[0] > 0 and 1 <= logits.shape[1] <= MAX_O
            and (tuple(target.shape) == (logits.shape[0],) or tuple(target.shape) == (logits.shape[0], 1)))


class _Og3dCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        B, O = logits.shape
        x = logits if logits.dtype == torch.float32 else logits.float()
        if x.stride(1) != 1 or (B > 1 and x.stride(0) < O) or x.data_ptr() % 4:
            x = x.contiguous()
        tgt = target.reshape(B).contiguous()
        dev = x.device
        f = dict(dtype=torch.float32, device=dev)
        loss, unit = torch.empty(1, **f), torch.empty((B, O), **f)
        partial = torch.empty(int(_native.load().gps_og3d_ce_partial_floats(B)), **f)
        launch("gps_og3d_ce_forward", B, O, x, x.stride(0) if B > 1 else O, tgt, loss, unit, partial, _native.ticket(dev, "og3d_ce"),
               device=dev, label=f"og3d_ce_forward(B={B},O={O})", nbytes=8 * B * O + 8 * B, what="og3d_ce_forward")
        ctx.save_for_backward(unit)
        ctx.dtype = logits.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (unit,) = ctx.saved_tensors
        return (unit * g).to(ctx.dtype), None


def og3d_ce(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """F.cross_entropy(logits (B, O), target (B,) or (B, 1) int64) as one fp32 device scalar; -inf logits allowed."""
    return _Og3dCE.apply(logits, target)
