"""Frozen bits of the LayerNorm partial-row reduction (csrc/gps_layernorm.hip): a SHA-256 of the raw output bytes of

  single/scratch   gps_ln_reduce_partials with its scratch (row slices + the last-arrival hand-off)
  single/plain     the same call without scratch (one workgroup per column group sums every row)
  grouped/acc=A    gps_ln_reduce_partials_grouped, A = 0 (stored over) / 1 (added to) a preset gamma / beta buffer; the
                   six `parts` of a width are the six problems of ONE launch, so the launch has as many slice rows as
                   its largest problem and the workgroups a smaller problem does not need leave at once

for parts in PARTS -- one slice (1, 63, 64), the 1 -> 2 slice boundary (65), an uneven last slice (130), more than
16 * 64 rows so that the slice cap is hit (1030) -- and d in DS (2 d = 640 is no multiple of the 64 columns of a
workgroup: the last column group is partial), written to tests/golden/ln_reduce_digests.json.  The summation order is
fixed (8 accumulators per thread, wave order, slice order), so a restatement of the kernels that moves no arithmetic
leaves every digest as it is; tests/test_gpu_fused_norm.py recomputes them.  Run it on a library whose kernels are known
good (the digests in the tree were recorded from the kernels as they were before the two shared one device body):

    python tests/golden/make_golden_ln_reduce.py [--out tests/golden/ln_reduce_digests.json]
"""
import argparse
import functools
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "ln_reduce_digests.json")

PARTS = [1, 63, 64, 65, 130, 1030]
DS = [256, 320]
FORMS = ["single/scratch", "single/plain", "grouped/acc=0", "grouped/acc=1"]
RED_SLICES, GROUP_MAX = 16, 64           # kRedSlices, kLnRedMax of the kernel file: the scratch layouts


def key(form, parts, d):
    return f"{form}/parts={parts}/d={d}"


def keys():
    return [key(f, p, d) for f in FORMS for d in DS for p in PARTS]


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def inputs(parts, d):
    """(part (2, parts, d), preset (2, d)) on the GPU, the same values on every call."""
    import torch
    g = torch.Generator().manual_seed(1000 * parts + d)
    return torch.randn(2, parts, d, generator=g).cuda(), torch.randn(2, d, generator=g).cuda()


def _zeros_bytes(nbytes):
    import torch
    return torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device="cuda")


def run_single(parts, d, with_scratch):
    """-> (out (2, d), the scratch's ticket words or None)"""
    import torch
    from sceneverse_amd import _native
    lib = _native.load()
    part, _ = inputs(parts, d)
    out = torch.full((2, d), float("nan"), device="cuda")
    scratch = _zeros_bytes(int(lib.gps_ln_reduce_scratch_bytes(d))) if with_scratch else None
    st = lib.gps_ln_reduce_partials(parts, d, part.data_ptr(), out.data_ptr(), scratch.data_ptr() if with_scratch else None,
                                    torch.cuda.current_stream().cuda_stream)
    _native.check(st, "ln_reduce_partials")
    torch.cuda.synchronize()
    return out, (scratch[RED_SLICES * 2 * d:] if with_scratch else None)


@functools.lru_cache(maxsize=None)
def run_grouped(d, accumulate):
    """One launch over the six problems of width d -> ({parts: out (2, d)}, the scratch's ticket words)"""
    import torch
    from sceneverse_amd import _native
    lib = _native.load()
    outs = {p: inputs(p, d)[1].clone() for p in PARTS}
    probs = []
    for p in PARTS:
        q = _native.LnReduceProblem()
        q.part, q.out_gamma, q.out_beta = inputs(p, d)[0].data_ptr(), outs[p][0].data_ptr(), outs[p][1].data_ptr()
        q.parts, q.accumulate = p, accumulate
        probs.append(q)
    scratch = _zeros_bytes(int(lib.gps_ln_reduce_grouped_scratch_bytes(d)))
    arr = (_native.LnReduceProblem * len(probs))(*probs)
    st = lib.gps_ln_reduce_partials_grouped(arr, len(probs), d, scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _native.check(st, "ln_reduce_partials_grouped")
    torch.cuda.synchronize()
    return outs, scratch[GROUP_MAX * RED_SLICES * 2 * d:]


def compute(form, parts, d):
    """(out, ticket words or None) of one case"""
    if form.startswith("single/"):
        return run_single(parts, d, form == "single/scratch")
    outs, tickets = run_grouped(d, int(form[-1]))
    return outs[parts], tickets


def load():
    with open(GOLDEN) as fh:
        return json.load(fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    got = {key(f, p, d): sha(compute(f, p, d)[0]) for f in FORMS for d in DS for p in PARTS}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(got, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(got)} digests to {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
