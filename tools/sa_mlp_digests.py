"""Frozen bits of the fused set-abstraction levels: a SHA-256 of the raw output bytes (sentinel rows of objects past the
device-side extent included) of every case of tests/test_gpu_sa_distinct.py --

  bf16x3   level (sa1, sa2) x the five PATTERNS x entry (channel-major; point-major where the level has it) x products
           (3, 1) x distinct (0 = dense kernel, 2 = distinct-sample kernel)
  fp32     gps_sa_mlp_forward on the all_distinct and mixed cases of both levels

-- written to tests/golden/sa_mlp_digests.json.  Both forms are deterministic (fixed MFMA order, an order-independent
integer max), so a change of gps_sa_mlp.hip that moves no arithmetic leaves every digest as it is; the parametrised test
of tests/test_gpu_sa_distinct.py recomputes them.  Run it on a library whose kernels are known good:

    python tools/sa_mlp_digests.py [--out tests/golden/sa_mlp_digests.json]

The cases, their seeds and the launches are the test file's own (_level_inputs, _idx via _build_cases, _run)."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sa_mlp_digests.json")

LEVEL_ENTRIES = [("sa2", "cm"), ("sa1", "cm"), ("sa1", "pm")]
PATTERNS = ["one_distinct", "all_distinct", "mixed", "not_a_prefix", "extent"]
FP32_PATTERNS = ["all_distinct", "mixed"]


def keys():
    out = [f"bf16x3/{level}/{pattern}/{entry}/products={products}/distinct={distinct}"
           for level, entry in LEVEL_ENTRIES for pattern in PATTERNS for products in (3, 1) for distinct in (0, 2)]
    return out + [f"fp32/{level}/{pattern}" for level in ("sa2", "sa1") for pattern in FP32_PATTERNS]


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _run_fp32(T, level, case):
    import torch
    from sceneverse_amd import _native
    from sceneverse_amd.pointnet2 import _ext
    (xyz, new_xyz, feats), idx, _, ch, _ = case
    b, n, npoint, c, _ = T.SHAPES[level]
    _, _, _, ws, shifts = T._level_inputs(level)
    wpack = _ext.sa_mlp_pack([w.to(xyz.device) for w in ws], [s.to(xyz.device) for s in shifts], "fp32")
    out = torch.full((b, ch[2], npoint), T.SENTINEL, dtype=torch.float32, device=xyz.device)
    st = _native.load().gps_sa_mlp_forward(b, n, npoint, 32, c, *ch, xyz.data_ptr(), new_xyz.data_ptr(), feats.data_ptr(),
                                           idx.data_ptr(), wpack.data_ptr(), out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    _native.check(st, "sa_mlp_forward")
    torch.cuda.synchronize()
    return out


def compute(key, cases, T):
    """The digest of one key; `cases` is T._build_cases(), T the module of tests/test_gpu_sa_distinct.py."""
    from sceneverse_amd import _native
    parts = key.split("/")
    if parts[0] == "fp32":
        return _sha(_run_fp32(T, parts[1], cases[parts[1], parts[2]]))
    _, level, pattern, entry, products, distinct = parts
    lib = _native.load()
    extent = T.SHAPES[level][0] - 1 if pattern == "extent" else None
    try:
        lib.gps_sa_mlp_set_products(int(products.split("=")[1]))
        lib.gps_sa_mlp_set_distinct(int(distinct.split("=")[1]))
        return _sha(T._run(level, cases[level, pattern], entry, extent))
    finally:
        lib.gps_sa_mlp_set_products(3)
        lib.gps_sa_mlp_set_distinct(1)


def load():
    with open(GOLDEN) as fh:
        return json.load(fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import test_gpu_sa_distinct as T
    cases = T._build_cases()
    got = {k: compute(k, cases, T) for k in keys()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(got, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {len(got)} digests to {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
