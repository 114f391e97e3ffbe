"""What every call on a resident store (`gpu_objects.PackedScans`, `gpu_text.PackedTexts`) does on the host before its
one launch, stated once: the two guards, the `out=` contract, the seed word.  `what` is the public function's name and
`noun` the store's contents ("scans", "texts"), for the messages.

The `out=` contract: a dict of preallocated tensors under the result's names, each contiguous, of the result's shape
and dtype and on the store's device; the launch writes them IN PLACE and the result dict holds those very tensors.  A
flag output (bool) may be a uint8 buffer instead: the kernels write bytes 0 / 1, and the result is its bool view.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence, Tuple

import torch

_FLAGS = (torch.bool, torch.uint8)               # one byte per flag either way


def need_finalized(store, what: str) -> None:
    """`store`: the device array finalize() creates (None before it)."""
    if store is None:
        raise RuntimeError(f"{what}.finalize() has not been called")


def need_gpu(dev: torch.device, what: str, noun: str) -> None:
    if dev.type != "cuda":
        raise RuntimeError(f"{what} runs on libgps_hip.so: {noun} must live on a GPU (no CPU path)")


def outputs(what: str, spec: Sequence[Tuple[str, torch.dtype, tuple]], out: Optional[dict], dev: torch.device,
            noun: str) -> dict:
    """spec: (name, dtype, shape) of every output -> {name: tensor}: allocated on `dev` when `out` is None, else out's
    own tensors after the check of the contract above (ValueError naming the output; a missing name is the same error)."""
    if out is None:
        return {name: torch.empty(shape, dtype=dt, device=dev) for name, dt, shape in spec}
    res = {}
    for name, dt, shape in spec:
        t = out.get(name)
        dtypes = _FLAGS if dt in _FLAGS else (dt,)
        if t is None or t.shape != shape or t.dtype not in dtypes or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{what}: out[{name!r}] must be a contiguous {tuple(shape)} {dt} tensor on the {noun}' GPU")
        res[name] = t
    return res


def as_bool(res: dict, names: Iterable[str]) -> dict:
    """The flag outputs as bool: a uint8 buffer becomes its bool view (same storage), a bool one stays the same object."""
    for name in names:
        if name in res and res[name].dtype != torch.bool:
            res[name] = res[name].view(torch.bool)
    return res


def seed_word(what: str, seed_dev: Optional[torch.Tensor], dev: torch.device, noun: str) -> None:
    if seed_dev is not None and (seed_dev.device != dev or seed_dev.dtype != torch.int64 or seed_dev.numel() != 1):
        raise ValueError(f"{what}: seed_dev must be one int64 word on the {noun}' GPU")


def u64(seed: int) -> int:
    return int(seed) & ((1 << 64) - 1)
