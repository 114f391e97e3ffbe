"""Compile every HIP source of libgps_hip.so to gfx950 assembly and list, per kernel, what the source does not show:
VGPRs, scratch bytes and scratch instructions (register arrays indexed at run time, spills), v_readfirstlane counts
(VGPR-resident descriptors -> waterfall loops around buffer loads), full-drain waits (`s_waitcnt vmcnt(0)`) and IEEE
division sequences (`v_div_scale_f32`: `1.f / x` and `__frcp_rn` are ~10 instructions, `__builtin_amdgcn_rcpf` is one).

    python tools/asm_audit.py [--out profiles/r4/asm_audit.txt] [file.hip ...]

Round 4 found three kernels losing 15 - 50 % this way; no GPU needed.

    python tools/asm_audit.py --digest [--out profiles/r7/isa_digest.txt] [file.hip ...]

prints instead, per kernel, a SHA-256 of its instructions and one of its `.amdhsa_kernel` descriptor (registers, LDS,
scratch), compiled with build.py's flags: two trees whose tables agree run the same device code, so a refactor of
`__forceinline__` helpers can be shown to have moved nothing.  Comment lines, the function index in local labels (a
kernel's position in its file), `__hip_cuid_*` (a hash of the source text), `.file` and `.ident` do not count."""
import argparse
import glob
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def demangle(names):
    try:
        out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt"], input="\n".join(names), capture_output=True, text=True).stdout
        return out.splitlines()
    except OSError:
        return names


def compile_asm(path, tmp, flags=None):
    asm = os.path.join(tmp, os.path.basename(path) + ".s")
    flags = flags or ["--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include"]
    subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", "-o", asm, path], check=True,
                   stderr=subprocess.DEVNULL)
    with open(asm) as fh:
        return fh.read()


def functions(text):
    """(mangled name, instructions, descriptor block) of every kernel: the whole function from its label to its
    `.Lfunc_end` (a kernel with an early exit has more than one s_endpgm), the `.amdhsa_kernel` block cut out of it."""
    out = []
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        d = re.search(r"^\s*\.amdhsa_kernel[^\n]*\n.*?\.end_amdhsa_kernel[^\n]*\n", m.group(2), re.S | re.M)
        if d:
            out.append((m.group(1), m.group(2)[:d.start()] + m.group(2)[d.end():], d.group(0)))
    return out


def build_flags(path):
    """COMMON plus the file's extra flags, read from sceneverse_amd/csrc/build.py; the source tree's csrc/ is on the
    include path so that a copy of a file elsewhere still finds the internal headers."""
    csrc = os.path.join(ROOT, "sceneverse_amd", "csrc")
    spec = importlib.util.spec_from_file_location("gps_csrc_build", os.path.join(csrc, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return [*b.COMMON, *dict(b.SOURCES).get(os.path.basename(path), []), "-I" + csrc]


def _sha(block):
    keep = [re.sub(r"\.(LBB|LJTI|Ltmp|Lfunc_begin|Lfunc_end)\d+", r".\1", ln.rstrip()) for ln in block.splitlines()
            if ln.strip() and not ln.lstrip().startswith(";")
            and not re.match(r"\s*\.(file|ident)\b", ln) and "__hip_cuid_" not in ln]
    return hashlib.sha256("\n".join(keep).encode()).hexdigest()


def digest(path, tmp):
    """[(mangled name, sha256 of the instructions, sha256 of the descriptor)], sorted by name."""
    return sorted((n, _sha(body), _sha(desc)) for n, body, desc in functions(compile_asm(path, tmp, build_flags(path))))


def audit(path, tmp):
    text = compile_asm(path, tmp)
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)(?=\n\s+- \.agpr_count|\n\s+- \.args|\Z)", text, re.S):
        blk = m.group(2)
        g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) if re.search(rf"\.{k}:\s+(\d+)", blk) else -1
        meta[m.group(1)] = (g("vgpr_count"), g("private_segment_fixed_size"), g("sgpr_spill_count"), g("vgpr_spill_count"))
    rows = []
    for name, body, _ in functions(text):
        if name not in meta:
            continue
        rows.append((name, *meta[name], len(re.findall(r"\bscratch_", body)), len(re.findall(r"v_readfirstlane", body)),
                     len(re.findall(r"s_waitcnt vmcnt\(0\)", body)), len(re.findall(r"v_mfma", body)),
                     len(re.findall(r"v_div_scale_f32", body)) // 2))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--digest", action="store_true", help="print per-kernel hashes of the device code instead")
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    files = a.files or sorted(glob.glob(os.path.join(ROOT, "sceneverse_amd", "csrc", "*.hip")))
    with tempfile.TemporaryDirectory() as tmp:
        if a.digest:
            from concurrent.futures import ThreadPoolExecutor
            lines = ["# sha256(instructions)  sha256(.amdhsa_kernel descriptor)  kernel"]
            with ThreadPoolExecutor(max_workers=min(len(files), 16)) as pool:
                for f, rows in zip(files, pool.map(lambda f: digest(f, tmp), files)):
                    lines.append(f"-- {os.path.relpath(f, ROOT)}")
                    lines += [f"{body}  {desc}  {name}" for name, body, desc in rows]
        else:
            lines = [f"{'vgpr':>5} {'scr_B':>6} {'s_sp':>4} {'v_sp':>4} {'scr_i':>5} {'rfl':>4} {'vm0':>4} {'mfma':>5} {'div':>4}  kernel"]
            for f in files:
                rows = audit(f, tmp)
                names = demangle([r[0] for r in rows])
                lines.append(f"-- {os.path.relpath(f, ROOT)}")
                for r, n in zip(rows, names):
                    lines.append(f"{r[1]:5d} {r[2]:6d} {r[3]:4d} {r[4]:4d} {r[5]:5d} {r[6]:4d} {r[7]:4d} {r[8]:5d} {r[9]:4d}  {n[:150]}")
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(out)


if __name__ == "__main__":
    main()
