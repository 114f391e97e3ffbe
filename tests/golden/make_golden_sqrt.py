"""Generate tests/golden/pairwise_sqrt_ref_host.pt: every square root that oracle.gps_torch_reference.calc_pairwise_locs
takes on the `obj_locs` of tests/golden/gps_reference_cpu.pt, as torch's CPU sqrt returned them on a host that
reproduces that fixture's `pairwise_locs` bit for bit (torch's CPU sqrt goes through MKL's vector math, whose last bit
depends on the host CPU).  tests/test_oracle_vs_golden.py::test_pairwise_locs_bit_exact answers from this table on
hosts whose roots differ.

    python tests/golden/make_golden_sqrt.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle import gps_torch_reference as R  # noqa: E402


def main():
    fx = torch.load(os.path.join(HERE, "gps_reference_cpu.pt"), weights_only=False)
    seen, real = [], torch.sqrt

    def recording_sqrt(t):
        out = real(t)
        seen.append((t.detach().reshape(-1).clone(), out.detach().reshape(-1).clone()))
        return out

    torch.sqrt = recording_sqrt
    try:
        got = R.calc_pairwise_locs(fx["batch"]["obj_locs"][:, :, :3])
    finally:
        torch.sqrt = real
    if not torch.equal(got, fx["pairwise_locs"]):
        raise SystemExit("this host does not reproduce gps_reference_cpu.pt's pairwise_locs: its roots are not the fixture's")
    x = torch.cat([a for a, _ in seen])
    r = torch.cat([b for _, b in seen])
    x, order = torch.sort(x)
    r = r[order]
    keep = torch.ones_like(x, dtype=torch.bool)
    keep[1:] = x[1:] != x[:-1]
    torch.save({"x": x[keep].contiguous(), "sqrt": r[keep].contiguous()}, os.path.join(HERE, "pairwise_sqrt_ref_host.pt"))
    print("roots:", int(keep.sum()))


if __name__ == "__main__":
    main()
