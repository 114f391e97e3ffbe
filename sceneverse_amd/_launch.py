"""The one way a Python wrapper launches a kernel of libgps_hip.so: `launch()` resolves the entry point, turns tensors
into addresses, enters the device of the tensors, appends THAT device's current stream, optionally brackets the call with
two timing events, and checks the status.  Also here: the per-launch profile that bench.py --full and the tests read
(`profile_start` / `profile_stop`; pointnet2/_ext.py re-exports them under their historical names).

`_native.py` stays the ctypes-only binding and does not import this module.  Functions of the library that launch nothing
(`gps_*_partial_rows`, `*_scratch_bytes`, `*_ws_floats`, `gps_gemm_pick_*`, the `gps_attn_set_*` / `gps_sa_mlp_set_*`
switches, `gps_point_set_object_extent`) are called directly: they take no stream.  Every launching entry point of
include/gps_hip.h takes its stream as the last parameter, so no launch site is left outside `launch()`.
"""
from __future__ import annotations

import torch

from . import _native

# ---- optional per-launch timing (bench.py): HIP events on the launch stream ------------------
_PROFILE = None  # None | {op name: [(start_event, end_event, algorithmic_bytes), ...]}


def profile_start() -> None:
    global _PROFILE
    _PROFILE = {}


def profiling() -> bool:
    return _PROFILE is not None


def profile_stop() -> dict:
    """-> {op: {"launches": n, "avg_us": t, "bytes_per_launch": B, "flops_per_launch": F,
    "mfma_dtype": "fp32"|"bf16"|None}} (synchronises)."""
    global _PROFILE
    rec, _PROFILE = _PROFILE or {}, None
    torch.cuda.synchronize()
    out = {}
    for name, evs in rec.items():
        ms = [s.elapsed_time(e) for s, e, *_ in evs]
        # launches with a device-side extent (gps_gemm_args.extent_dev) did only `frac` of the work their static
        # shape names: the snapshot of the extent word taken at launch time is read back here, once
        fr = [ev[5]() if ev[5] is not None else 1.0 for ev in evs]
        out[name] = {"launches": len(evs), "avg_us": 1e3 * sum(ms) / len(ms),
                     "bytes_per_launch": sum((ev[2](f) if callable(ev[2]) else ev[2] * f) for ev, f in zip(evs, fr)) / len(evs),
                     "flops_per_launch": sum(ev[3] * f for ev, f in zip(evs, fr)) / len(evs),
                     "mfma_dtype": evs[0][4]}
        if any(ev[5] is not None for ev in evs):
            out[name]["work_fraction"] = sum(fr) / len(fr)
    return out


class _timed:
    """Brackets one native launch with two events on the current (= launch) stream."""

    def __init__(self, name: str, algo_bytes: int, algo_flops: int = 0, mfma_dtype=None, work_fraction=None):
        """work_fraction: None, or a callable evaluated at profile_stop() -> the share of the static shape's
        algorithmic work this launch really did (device-side extents)."""
        self.name, self.bytes, self.flops, self.mfma = name, algo_bytes, algo_flops, mfma_dtype
        self.work_fraction = work_fraction

    def __enter__(self):
        if _PROFILE is not None:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *exc):
        if _PROFILE is not None:
            self.e.record()
            _PROFILE.setdefault(self.name, []).append((self.s, self.e, self.bytes, self.flops, self.mfma,
                                                       self.work_fraction))
        return False


# ---- the launch -----------------------------------------------------------------------------------------------------
def ptr(t):
    """Address of an optional tensor: None stays None (a null pointer of the C ABI)."""
    return None if t is None else t.data_ptr()


def c_arg(a):
    """One argument of a native call: a tensor goes as its address; None, numbers and ctypes objects (a `byref(struct)`,
    a struct array) go as they are."""
    return a.data_ptr() if isinstance(a, torch.Tensor) else a


def launch(name: str, *args, device, label=None, nbytes=None, flops=0, mfma=None, work_fraction=None, accept=(),
           what=None) -> int:
    """Call entry point `name` of libgps_hip.so with `args` (mapped by `c_arg`) and, as the last argument, the current
    stream of `device` -- the device of the tensors launched on -- with that device current.
    nbytes: None = no profile record; else the launch is timed under the key `label` (default: `name` without its
    `gps_` prefix) with this algorithmic byte count and `flops` / `mfma` / `work_fraction` (see `_timed`).
    -> the status, when it is GPS_OK or listed in `accept` (a site that treats GPS_ERR_UNSUPPORTED as an answer);
    any other status raises through `_native.check` with the text `what` (default: the profile key)."""
    fn = getattr(_native.load(), name)
    key = label or name[4:]
    argv = [c_arg(a) for a in args]
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        if nbytes is None:
            status = fn(*argv, stream)
        else:
            with _timed(key, nbytes, flops, mfma, work_fraction):
                status = fn(*argv, stream)
    if status != _native.GPS_OK and status not in accept:
        _native.check(status, what or key)
    return status
