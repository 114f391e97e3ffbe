"""Ranked top-k answers and their hit counts on libgps_hip.so (gps_answer_hits, gps_answer_fold; csrc/gps_metrics.hip):
the tensor side of the two entries, used by the ScanQA / SQA3D counters of engine.py.  GPU tensors only -- there is no
CPU path.

The ranking law (include/gps_hip.h): NaN above every number, then the value descending with -0.0 == +0.0, among equals
the lower answer id first -- torch.argmax's rule at every place."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from .. import _launch, _native
from .._launch import ptr

WORDS = _native.ANSWER_WORDS          # hit1, hitk, count, type_hit1[8], type_count[8]
_LABEL_KINDS = {torch.int64: 0, torch.uint8: 1, torch.float32: 2}


def _matrix(x: torch.Tensor, what: str) -> torch.Tensor:
    """(rows, V) with unit column stride and a row pitch >= V (copied only when it is not)."""
    if x.dim() != 2 or x.shape[1] == 0:
        raise ValueError(f"answer_hits: {what} must be (rows, V) with V > 0, not {tuple(x.shape)}")
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x


def hits(scores: torch.Tensor, label: torch.Tensor, words: torch.Tensor, k: int = 10, *,
         types: Optional[torch.Tensor] = None, n_types: int = 0, rows_dev: Optional[torch.Tensor] = None,
         topk: Optional[torch.Tensor] = None) -> None:
    """ONE gps_answer_hits launch on the current stream: adds the batch into `words` (19 contiguous int64) and, with
    `topk` ((rows, k) contiguous int32), writes each live row's k best answer ids in rank order (-1 past V).
    scores (rows, V) f32 / bf16 (other float types go through fp32); label (rows, V) int64, bool / uint8 or f32, an
    entry counts iff it equals 1; types (rows) int64 with n_types <= 8; rows_dev: one int32 word, the live row count."""
    if scores.device.type != "cuda":
        raise RuntimeError("answer_hits runs on libgps_hip.so: the scores must live on a GPU (no CPU path)")
    if scores.dtype not in (torch.float32, torch.bfloat16):
        if not scores.is_floating_point():
            raise ValueError(f"answer_hits: scores must be a floating-point tensor, not {scores.dtype}")
        scores = scores.float()
    x = _matrix(scores, "scores")
    rows, V = x.shape
    if label.dtype == torch.bool:
        label = label.view(torch.uint8) if label.is_contiguous() else label.contiguous().view(torch.uint8)
    elif label.dtype not in _LABEL_KINDS:
        label = label.to(torch.float32) if label.is_floating_point() else label.to(torch.int64)
    lab = _matrix(label, "label")
    if tuple(lab.shape) != (rows, V):
        raise ValueError(f"answer_hits: label {tuple(lab.shape)} for scores {(rows, V)}")
    if words.dtype != torch.int64 or words.numel() != WORDS or not words.is_contiguous():
        raise ValueError(f"answer_hits: words must be {WORDS} contiguous int64 words")
    if types is not None:
        types = types.reshape(-1)
        if types.dtype != torch.int64 or not types.is_contiguous():
            types = types.to(torch.int64).contiguous()
        if types.numel() != rows:
            raise ValueError(f"answer_hits: {types.numel()} types for {rows} rows")
    if rows_dev is not None and (rows_dev.dtype != torch.int32 or rows_dev.numel() != 1):
        raise ValueError("answer_hits: rows_dev must be one int32 word")
    if topk is not None and (topk.dtype != torch.int32 or tuple(topk.shape) != (rows, k) or not topk.is_contiguous()):
        raise ValueError(f"answer_hits: topk must be contiguous int32 {(rows, k)}")
    for t in (lab, words, types, rows_dev, topk):
        if t is not None and t.device != x.device:
            raise ValueError("answer_hits: label, types, extent, topk and words must live on the scores' GPU")
    a = _native.AnswerHitsArgs(
        rows=rows, cols=V, scores=x.data_ptr(), ld=x.stride(0) if rows > 1 else V,
        scores_bf16=int(x.dtype == torch.bfloat16), label_kind=_LABEL_KINDS[lab.dtype], label=lab.data_ptr(),
        ld_label=lab.stride(0) if rows > 1 else V, type=ptr(types), n_types=int(n_types) if types is not None else 0,
        k=int(k), rows_dev=ptr(rows_dev), topk=ptr(topk), words=words.data_ptr())
    _launch.launch("gps_answer_hits", ctypes.byref(a), device=x.device)


def _f64(t: Optional[torch.Tensor], n: int, what: str) -> None:
    if t is None or t.dtype != torch.float64 or t.numel() < n or not t.is_contiguous() or t.device.type != "cuda":
        raise ValueError(f"answer_fold: {what} must be a contiguous float64 GPU tensor of at least {n} entries")


def fold_pairs(words: torch.Tensor, cls_words: Optional[torch.Tensor], n_cls: int, sums: torch.Tensor,
               last: torch.Tensor) -> None:
    """ONE gps_answer_fold launch, integer pairs: (hit1, count), (hitk, count) and the first n_cls rows of `cls_words`
    ((n, 6) int64 gps_cls_hits counters) are added into `sums` (2 * (2 + n_cls) int64) and cleared; last[p] = h / max(c, 1)."""
    _f64(last, 2 + n_cls, "last")
    if sums.dtype != torch.int64 or sums.numel() < 2 * (2 + n_cls) or not sums.is_contiguous():
        raise ValueError("answer_fold: sums must be contiguous int64, two words per pair")
    _launch.launch("gps_answer_fold", words, cls_words if n_cls else None, int(n_cls), 0, ctypes.c_double(1.0), sums, last,
                   None, None, None, device=words.device)


def fold_sqa3d(words: torch.Tensor, cls_words: Optional[torch.Tensor], n_types: int, weight: float, last: torch.Tensor,
               acc: torch.Tensor, type_total: torch.Tensor, total: torch.Tensor) -> None:
    """ONE gps_answer_fold launch, SQA3DEval's float64 bookkeeping (include/gps_hip.h): last (4 + 2 n_types), acc
    (4 + n_types), type_total (n_types, started at 1e-10 by the caller), total (1); `cls_words`: the 6 counters of the
    obj_cls_raw problem or None."""
    _f64(last, 4 + 2 * n_types, "last")
    _f64(acc, 4 + n_types, "acc")
    _f64(type_total, n_types, "type_total")
    _f64(total, 1, "total")
    _launch.launch("gps_answer_fold", words, cls_words, int(cls_words is not None), int(n_types),
                   ctypes.c_double(float(weight)), None, last, acc, type_total, total, device=words.device)
