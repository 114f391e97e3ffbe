"""Summed BCE-with-logits losses on libgps_hip.so: one launch per direction each.

Reference: optim/loss/loss.py:50-53 (answer_loss: the .float() cast of the (B, 8864) int64 labels and
binary_cross_entropy_with_logits(reduction='sum') / B) -> `bce_logits_sum` (csrc/gps_qa.hip), and
optim/loss/contra_loss.py:29-35 (TextObjWithinBatch with task ScanQA: two normalisations, an einsum and a weighted BCE)
-> `text_obj_bce` (csrc/gps_contrastive.hip, the sibling of fused_contra.text_obj_ce).  The integer targets are read in
place.  GPU tensors only; the callers keep the torch composition for anything else."""
from __future__ import annotations

from typing import Optional

import torch

from ... import _native
from ..._launch import launch
from .fused_contra import _LDS_LIMIT, _rows_ok


def bce_logits_usable(x: torch.Tensor, y: torch.Tensor, weight: Optional[torch.Tensor] = None) -> bool:
    return (x.is_cuda and y.is_cuda and x.dim() == 2 and x.shape == y.shape and x.numel() > 0
            and x.dtype in (torch.bfloat16, torch.float32) and y.dtype in (torch.int64, torch.float32)
            and x.shape[0] * ((x.shape[1] + 7) // 8) < 2 ** 31
            and (weight is None or (weight.is_cuda and weight.shape == x.shape
                                    and weight.dtype in (torch.bool, torch.uint8))))


class _BCELogitsSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, weight, scale: float):
        rows, cols = x.shape
        if x.stride(1) != 1:
            x = x.contiguous()
        y = y.contiguous()
        w8 = None if weight is None else weight.to(torch.uint8).contiguous()
        dev = x.device
        partial = torch.empty(int(_native.load().gps_bce_logits_partial_floats(rows, cols)), dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nbytes = x.numel() * x.element_size() + y.numel() * y.element_size() + (0 if w8 is None else w8.numel())
        launch("gps_bce_logits_forward", rows, cols, int(x.dtype == torch.bfloat16), x, x.stride(0), int(y.dtype == torch.float32),
               y, w8, float(scale), partial, loss, _native.ticket(dev, "bce_logits"), device=dev,
               label=f"bce_logits_forward(rows={rows},cols={cols})", nbytes=nbytes, what="bce_logits_forward")
        ctx.save_for_backward(x, y, *(() if w8 is None else (w8,)))
        ctx.scale = float(scale)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        x, y, *rest = ctx.saved_tensors
        w8 = rest[0] if rest else None
        rows, cols = x.shape
        g = g.reshape(1).float().contiguous()
        dx = torch.empty((rows, cols), dtype=x.dtype, device=x.device)
        nbytes = 2 * x.numel() * x.element_size() + y.numel() * y.element_size() + (0 if w8 is None else w8.numel())
        launch("gps_bce_logits_backward", rows, cols, int(x.dtype == torch.bfloat16), x, x.stride(0), int(y.dtype == torch.float32),
               y, w8, ctx.scale, g, dx, dx.stride(0), device=x.device, label=f"bce_logits_backward(rows={rows},cols={cols})",
               nbytes=nbytes, what="bce_logits_backward")
        return dx, None, None, None


def bce_logits_sum(x: torch.Tensor, y: torch.Tensor, weight: Optional[torch.Tensor] = None, scale: float = 1.0):
    """scale * sum(weight * BCEWithLogits(x, y)) as one fp32 device scalar; x (rows, cols) bf16 / fp32, y int64 / fp32,
    weight bool / uint8 or None."""
    return _BCELogitsSum.apply(x, y, weight, scale)


def text_obj_bce_usable(obj, text, labels, masks) -> bool:
    return (obj.dim() == 3 and text.dim() == 2 and _rows_ok(obj, text) and obj.shape[1] <= 4096
            and 4 * (obj.shape[2] + obj.shape[1] + 16) <= _LDS_LIMIT and labels.is_cuda and masks.is_cuda
            and labels.shape == obj.shape[:2] and labels.dtype == torch.int64
            and masks.shape == obj.shape[:2] and masks.dtype in (torch.bool, torch.uint8) and obj.shape[0] > 0
            and text.shape == (obj.shape[0], obj.shape[2]))


class _TextObjBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, obj, text, labels, masks, eps: float):
        B, O, D = obj.shape
        obj, text = obj.contiguous(), text.contiguous()
        labels = labels.contiguous()
        masks = masks.to(torch.uint8).contiguous()
        dev = obj.device
        f = dict(dtype=torch.float32, device=dev)
        cosv, coef, inv_o = torch.empty((B, O), **f), torch.empty((B, O), **f), torch.empty((B, O), **f)
        inv_t, loss_rows, scal = torch.empty(B, **f), torch.empty(B, **f), torch.empty(2, **f)
        launch("gps_text_obj_bce_forward", B, O, D, obj, text, labels, masks, float(eps), cosv, coef, inv_o, inv_t, loss_rows,
               scal, _native.ticket(dev, "text_obj_bce"), device=dev, label=f"text_obj_bce_forward(B={B},O={O},D={D})",
               nbytes=4 * (obj.numel() + text.numel()), what="text_obj_bce_forward")
        ctx.save_for_backward(obj, text, cosv, coef, inv_o, inv_t, scal)
        ctx.eps = float(eps)
        return scal[0]

    @staticmethod
    def backward(ctx, g):
        obj, text, cosv, coef, inv_o, inv_t, scal = ctx.saved_tensors
        B, O, D = obj.shape
        g = g.reshape(1).float().contiguous()
        dobj = torch.empty_like(obj) if ctx.needs_input_grad[0] else None
        dtext = torch.empty_like(text) if ctx.needs_input_grad[1] else None
        launch("gps_text_obj_bce_backward", B, O, D, obj, text, ctx.eps, cosv, coef, inv_o, inv_t, scal, g, dobj, dtext,
               device=obj.device, label=f"text_obj_bce_backward(B={B},O={O},D={D})", nbytes=8 * obj.numel(),
               what="text_obj_bce_backward")
        return dobj, dtext, None, None, None


def text_obj_bce(obj, text, labels, masks, eps: float = 1e-12):
    """sum_bo masks * BCEWithLogits(<normalize(obj[b, o]), normalize(text[b])>, labels[b, o]) / B -- TextObjWithinBatch's
    BCE branch."""
    return _TextObjBCE.apply(obj, text, labels, masks, eps)
