"""Row arg-max / hit counts on libgps_hip.so (gps_cls_hits, gps_metrics_fold; csrc/gps_metrics.hip): the tensor side of
the two entries, shared by the device-side evaluators of engine.py and the masked-LM hit count of
optim/loss/fused_lm_loss.py.  GPU tensors only -- there is no CPU path."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .. import _launch, _native
from .._launch import ptr

WORDS = 6                         # hits, count, hits & a, count & a, hits & b, count & b


def _rows(logits: torch.Tensor):
    """(..., V) float tensor -> (2-D tensor with unit column stride and a row pitch >= V, rows, V)."""
    if logits.dtype not in (torch.float32, torch.bfloat16):
        if not logits.is_floating_point():
            raise ValueError(f"cls_hits: logits must be a floating-point tensor, not {logits.dtype}")
        logits = logits.float()                     # fp16 / fp64 -> fp32 (fp16 exactly: the arg-max is unchanged)
    V = logits.shape[-1]
    x = logits.reshape(-1, V)
    if V == 0:
        raise ValueError("cls_hits: logits without columns")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < V):
        x = x.contiguous()
    return x, x.shape[0], V


def _mask(m: Optional[torch.Tensor], rows: int, what: str):
    if m is None:
        return None
    if m.dtype == torch.bool:
        m = m.view(torch.uint8) if m.is_contiguous() else m.contiguous().view(torch.uint8)
    elif m.dtype not in (torch.uint8, torch.int64):
        m = (m != 0).view(torch.uint8)              # any other number type: nonzero = true
    m = m.reshape(-1)
    if not m.is_contiguous():
        m = m.contiguous()
    if m.numel() != rows:
        raise ValueError(f"cls_hits: {what} has {m.numel()} entries for {rows} rows")
    return m


def problem(logits: torch.Tensor, labels: torch.Tensor, counters: torch.Tensor, *, ignore_index: Optional[int] = None,
            rows_dev: Optional[torch.Tensor] = None, sel: Optional[torch.Tensor] = None,
            split_a: Optional[torch.Tensor] = None, split_b: Optional[torch.Tensor] = None, cols: Optional[int] = None):
    """One gps_cls_hits problem -> (struct, tensors the struct points into).  logits (..., V) f32 / bf16; labels, sel,
    split_a, split_b: one entry per row (any shape with rows entries); counters: 6 contiguous int64 words on the same
    GPU; cols: read only the first `cols` columns of each row (the padded vocabulary of the lazy masked-LM path)."""
    if logits.device.type != "cuda":
        raise RuntimeError("cls_hits runs on libgps_hip.so: the logits must live on a GPU (no CPU path)")
    x, rows, V = _rows(logits)
    dev = x.device
    cols = V if cols is None else int(cols)
    lab = labels.reshape(-1)
    if lab.dtype != torch.int64 or not lab.is_contiguous():
        lab = lab.to(torch.int64).contiguous()
    if lab.numel() != rows:
        raise ValueError(f"cls_hits: {lab.numel()} labels for {rows} rows")
    masks = [_mask(m, rows, n) for m, n in ((sel, "sel"), (split_a, "split_a"), (split_b, "split_b"))]
    sizes = {m.element_size() for m in masks if m is not None}
    if len(sizes) > 1:                               # one element size per problem: bring the int64 ones to bytes
        masks = [None if m is None else (m if m.element_size() == 1 else (m != 0).view(torch.uint8)) for m in masks]
        sizes = {1}
    if counters.dtype != torch.int64 or counters.numel() != WORDS or not counters.is_contiguous():
        raise ValueError("cls_hits: counters must be 6 contiguous int64 words")
    keep = [x, lab, counters, rows_dev] + masks
    for t in keep:
        if t is not None and t.device != dev:
            raise ValueError("cls_hits: labels, masks, extent and counters must live on the logits' GPU")
    if rows_dev is not None and (rows_dev.dtype != torch.int32 or rows_dev.numel() != 1):
        raise ValueError("cls_hits: rows_dev must be one int32 word")
    p = _native.ClsHitsProblem(
        rows=rows, cols=cols, logits=x.data_ptr(), ld=x.stride(0) if rows > 1 else V,
        logits_bf16=int(x.dtype == torch.bfloat16), use_ignore=int(ignore_index is not None),
        ignore_index=int(ignore_index or 0), labels=lab.data_ptr(), rows_dev=ptr(rows_dev), sel=ptr(masks[0]),
        split_a=ptr(masks[1]), split_b=ptr(masks[2]), mask_elem_bytes=sizes.pop() if sizes else 1, reserved=0,
        counters=counters.data_ptr())
    return p, keep


def launch(problems, device: torch.device) -> None:
    """ONE gps_cls_hits launch over `problems` (a list of `problem()` results) on the current stream of `device`."""
    if not problems:
        return
    if len(problems) > _native.CLS_HITS_MAX_PROBLEMS:
        raise ValueError(f"cls_hits: {len(problems)} problems in one launch (at most {_native.CLS_HITS_MAX_PROBLEMS})")
    arr = (_native.ClsHitsProblem * len(problems))(*[p for p, _ in problems])
    _launch.launch("gps_cls_hits", arr, len(problems), device=device)


def term(hits: torch.Tensor, count: Optional[torch.Tensor] = None, sub_hits: Optional[torch.Tensor] = None,
         sub_count: Optional[torch.Tensor] = None, eps: float = 0.0, const_denominator: Optional[float] = None):
    """One gps_metric_term over 1-element views of the counter words."""
    return _native.MetricTerm(hits=ptr(hits), count=ptr(count), sub_hits=ptr(sub_hits), sub_count=ptr(sub_count),
                              eps=float(eps), const_denominator=float(const_denominator or 0.0),
                              use_const_denominator=int(const_denominator is not None), reserved=0)


def fold(terms, weight: float, n_mean: int, last: torch.Tensor, acc: torch.Tensor, total: torch.Tensor) -> None:
    """ONE gps_metrics_fold launch: last / acc (len(terms) + 1 float64), total (1 float64) on the current stream."""
    for t, n in ((last, len(terms) + 1), (acc, len(terms) + 1), (total, 1)):
        if t.dtype != torch.float64 or t.numel() < n or not t.is_contiguous() or t.device.type != "cuda":
            raise ValueError("metrics_fold: last / acc / total must be contiguous float64 GPU tensors")
    arr = (_native.MetricTerm * max(len(terms), 1))(*terms)
    _launch.launch("gps_metrics_fold", len(terms), arr, ctypes.c_double(float(weight)), int(n_mean), last, acc, total,
                   device=last.device)
