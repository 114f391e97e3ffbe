"""Column sums of a bf16 matrix on libgps_hip.so (gps_colsum_bf16): the bias gradient `dY.sum(0)` of a Linear
whose weight gradient does NOT go through gps_gemm_bf16's TN form (that form produces it from the same tiles)."""
from __future__ import annotations

import torch

from .. import _native
from .._launch import launch


def colsum_bf16(dy2: torch.Tensor) -> torch.Tensor:
    """(T, N) bf16 -> (N,) fp32 column sums, fp32 accumulation in a fixed order (deterministic)."""
    T, N = dy2.shape
    out = torch.empty(N, dtype=torch.float32, device=dy2.device)
    parts = _native.load().gps_colsum_parts(T, N)
    scratch = torch.empty((max(parts, 1), N), dtype=torch.float32, device=dy2.device)
    st = launch("gps_colsum_bf16", T, N, dy2, dy2.stride(0), scratch, out, device=dy2.device,
                label=f"colsum_bf16(rows={T},cols={N})", nbytes=2 * T * N + 4 * N, what="colsum_bf16",
                accept=(_native.GPS_ERR_UNSUPPORTED,))
    if st == _native.GPS_ERR_UNSUPPORTED:            # columns / pitch not a multiple of 8: not this kernel's shape
        return dy2.sum(0, dtype=torch.float32)
    return out
