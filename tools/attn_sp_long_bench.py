"""Spatial self-attention core at B = 64, H = 12: the plane form (gps_attention_sp.hip up to 144 rows,
gps_attention_spl.hip above) against the general kernels (interleaved fp32 pairwise tensor, gps_attention.hip) at
L = 144, 160, 256, 512.

One forward call and one backward call of the autograd Function each, timed with device events over `iters` back-to-back
calls after a warm-up; the two forms alternate `repeats` times per length, so that clock and thermal drift hit both.
Reports the median and the spread of the repeats, and the algorithmic bytes / FLOPs of fused_attention's own model.
    python tools/attn_sp_long_bench.py [--lengths 144,160,256,512] [--repeats 3] [--iters 10] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sceneverse_amd.modules.layers import fused_attention as FA  # noqa: E402
from sceneverse_amd.modules.layers.fused_attention import _FusedSelfAttention  # noqa: E402

B, H, D = 64, 12, 768
DEV = "cuda"


def timeit(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters                 # us per call


def one(packed, pl, mask, go, planes, iters):
    FA.set_spatial_planes(planes)
    try:
        with torch.no_grad():
            t_f = timeit(lambda: _FusedSelfAttention.apply(packed, pl, mask, H, 0.0, 0, None), iters)
        x = packed.detach().clone().requires_grad_(True)
        o = _FusedSelfAttention.apply(x, pl, mask, H, 0.0, 0, None)
        t_b = timeit(lambda: torch.autograd.grad(o, x, go, retain_graph=True), iters)
    finally:
        FA.set_spatial_planes(True)
    return t_f, t_b


def model(L, planes):
    """(forward bytes, backward bytes, forward FLOPs, backward FLOPs) as fused_attention._call reports them."""
    ld = (L + 3) // 4 * 4
    if planes:
        fb = 2 * B * L * 4 * D + B * 5 * L * ld * 2 + B * L * H * 6 * 2
        bb = 2 * B * L * 9 * D + B * 5 * L * ld * 2 + 2 * B * L * H * 6 * 2
    else:
        fb = 2 * B * L * 4 * D + B * L * L * 5 * 4 + B * L * H * 6 * 4
        bb = 2 * B * L * 8 * D + B * L * L * 5 * 4 + 2 * B * L * H * 6 * 4
    return fb, bb, 4 * B * H * L * L * 64, 10 * B * H * L * L * 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="144,160,256,512")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    rows = []
    for L in [int(v) for v in args.lengths.split(",")]:
        packed = torch.randn(B, L, 3 * D + 6 * H, device=DEV)
        packed[..., 3 * D:] *= 2.0
        packed = packed.to(torch.bfloat16)
        pl = torch.rand(B, L, L, 5, device=DEV) * 2 - 1
        n_real = torch.randint(max(1, L // 2), L + 1, (B,), device=DEV)
        mask = torch.arange(L, device=DEV)[None, :] >= n_real[:, None]
        go = torch.randn(B, L, D, device=DEV).to(torch.bfloat16)
        t = {True: ([], []), False: ([], [])}
        for _ in range(args.repeats):
            for planes in (False, True):                   # alternating
                f, b = one(packed, pl, mask, go, planes, args.iters)
                t[planes][0].append(f)
                t[planes][1].append(b)
        for planes in (False, True):
            fb, bb, ff, bf = model(L, planes)
            fw, bw = t[planes]
            row = {"L": L, "form": "planes" if planes else "general",
                   "fwd_us": round(statistics.median(fw), 1), "fwd_us_all": [round(v, 1) for v in fw],
                   "bwd_us": round(statistics.median(bw), 1), "bwd_us_all": [round(v, 1) for v in bw],
                   "fwd_bytes": fb, "bwd_bytes": bb, "fwd_flops": ff, "bwd_flops": bf,
                   "fwd_tflops": round(ff / statistics.median(fw) / 1e6, 1),
                   "bwd_tflops": round(bf / statistics.median(bw) / 1e6, 1)}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del packed, pl, mask, go
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
