"""In-process A/B of the fused SA levels: distinct-sample form (gps_sa_mlp_set_distinct(2): both levels) against the dense
form (0), alternating, on two kinds of clouds:

  full     every group of every level is full -- all 1024 points of an object within 0.2 of each other (SA1), its 32
           centres within 0.4 (SA2): nothing can be dropped, the distinct form may only cost its compaction;
  typical  the synthetic objects of the benchmark batch (data/synthetic.synth_object).

Indices come from the library's own FPS and ball query; the features of SA2 are random (the time does not depend on the
values).  Prints, per kind and level, the mean distinct samples per group and every repeat of both forms in us (each
repeat = one HIP-graph replay of `--iters` launches)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from kernel_bench import timeit  # noqa: E402
from sceneverse_amd.data.synthetic import synth_object  # noqa: E402
from sceneverse_amd.pointnet2 import _ext as hip  # noqa: E402


def clouds(kind, b, rng):
    if kind == "full":
        v = rng.normal(size=(b, 1024, 3))
        v *= (0.09 * rng.uniform(size=(b, 1024, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=2, keepdims=True)   # ball of radius 0.09
        return torch.from_numpy(v.astype(np.float32))
    return torch.from_numpy(np.stack([synth_object(rng, 1024)[:, :3] for _ in range(b)]))


def distinct_per_group(idx):
    return ((idx != idx[..., :1]).sum(-1) + 1).float().mean().item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(42)
    g = torch.Generator().manual_seed(0)
    packs = {}
    for lvl, (c, ch) in {"SA1": (3, (64, 64, 128)), "SA2": (128, (128, 128, 256))}.items():
        ws, shifts, c_in = [], [], 3 + c
        for c_out in ch:
            ws.append((torch.randn(c_out, c_in, generator=g) / c_in ** 0.5).to(dev))
            shifts.append((0.1 * torch.randn(c_out, generator=g)).to(dev))
            c_in = c_out
        packs[lvl] = (hip.sa_mlp_pack(ws, shifts, "bf16x3"), ch)
    rows = []
    for kind in ("full", "typical"):
        xyz = clouds(kind, args.objects, rng).to(dev)
        b = xyz.shape[0]
        _, c1 = hip.furthest_point_sampling_xyz(xyz, 32)
        i1 = hip.ball_query(c1, xyz, 0.2, 32)
        f1 = (torch.rand(b, 3, 1024, generator=g) * 2 - 1).to(dev)
        _, c2 = hip.furthest_point_sampling_xyz(c1, 16)
        i2 = hip.ball_query(c2, c1, 0.4, 32)
        f2 = torch.randn(b, 128, 32, generator=g).to(dev)
        for lvl, (x, ctr, f, idx) in {"SA1": (xyz, c1, f1, i1), "SA2": (c1, c2, f2, i2)}.items():
            wpack, ch = packs[lvl]
            fn = lambda: hip.sa_mlp_forward(x, ctr, f, idx, wpack, ch, "bf16x3")   # noqa: E731
            us = {0: [], 1: []}
            try:
                for _ in range(args.repeats):
                    for on in (0, 1):
                        hip.sa_mlp_set_distinct(2 * on)
                        us[on].append(timeit(fn, iters=args.iters))
                hip.sa_mlp_set_distinct(0)
                dense = fn()
                hip.sa_mlp_set_distinct(2)
                same = torch.equal(fn(), dense)
            finally:
                hip.sa_mlp_set_distinct(1)
            row = {"clouds": kind, "level": lvl, "objects": b, "distinct_per_group": distinct_per_group(idx),
                   "dense_us": us[0], "distinct_us": us[1], "equal": same}
            rows.append(row)
            print(f"{kind:8s} {lvl}  distinct/group {row['distinct_per_group']:5.2f}  dense " +
                  " ".join(f"{t:7.1f}" for t in us[0]) + "   distinct " + " ".join(f"{t:7.1f}" for t in us[1]) +
                  f"   equal={same}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
