"""What the compiler made of three kernels, checked on the assembly (no GPU needed; hipcc cross-compiles gfx950).

Round 4 found the fused LayerNorm, the word-table gradient and the grouped weight-gradient launch 15 - 50 % below their
design because of code that does not show in the source: loads serialised behind wave-uniform
branches, a register array sent to scratch by a dynamic `break`, VGPR-resident buffer descriptors that put every stage
copy of a GEMM main loop inside a waterfall loop.  These are the regressions a source review does not catch, so the
properties are pinned here with tools/asm_audit.py's parser."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


import functools


@functools.lru_cache(maxsize=None)
def _asm(name):
    tmp = tempfile.mkdtemp(prefix="gps_asm_")
    out = os.path.join(tmp, name + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", "-S", "--cuda-device-only",
                    "-o", out, os.path.join(ROOT, "sceneverse_amd", "csrc", name + ".hip")], check=True,
                   stderr=subprocess.DEVNULL)
    text = open(out).read()
    shutil.rmtree(tmp, ignore_errors=True)
    return text


def _kernel(text, pattern):
    """(body, metadata block) of the first kernel whose mangled name matches `pattern`."""
    m = re.search(rf"^(_Z\w*{pattern}\w*):[^\n]*\n(.*?)s_endpgm", text, re.S | re.M)
    assert m, pattern
    meta = re.search(rf"\.name:\s+{re.escape(m.group(1))}\n(.*?)(?=\n\s+- \.agpr_count|\n\s+- \.args|\Z)", text, re.S)
    assert meta, pattern
    return m.group(2), meta.group(1)


def _meta(block, key):
    return int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))


def test_audit_tool_parses_a_small_file():
    import asm_audit
    with tempfile.TemporaryDirectory() as tmp:
        rows = asm_audit.audit(os.path.join(ROOT, "sceneverse_amd", "csrc", "gps_embedding.hip"), tmp)
    names = [r[0] for r in rows]
    assert any("sum_kernel" in n for n in names) and any("mark_kernel" in n for n in names)
    for r in rows:
        assert r[1] > 0 and r[2] == 0 and r[5] == 0, r          # VGPRs reported, no scratch bytes, no scratch instructions


def test_word_table_gradient_keeps_its_rows_in_registers_and_its_loads_in_flight():
    body, meta = _kernel(_asm("gps_embedding"), "sum_kernel")
    assert _meta(meta, "private_segment_fixed_size") == 0 and "scratch_" not in body
    # the scan of the duplicate list (int32 token / id pairs): >= 16 global loads between two waits somewhere in the
    # kernel (was one load per wait)
    runs = [len(re.findall(r"global_load_dword\s", seg)) for seg in re.split(r"s_waitcnt vmcnt", body)]
    assert max(runs) >= 12, runs                                   # 2 x 8 list words per trip, all but a straggler together
    # the row fetch: 16 x 16-byte loads issued back to back
    runs4 = [len(re.findall(r"global_load_dwordx4", seg)) for seg in re.split(r"s_waitcnt vmcnt", body)]
    assert max(runs4) >= 16, runs4


def test_single_workgroup_compactions_keep_their_loads_in_flight():
    """compact_ranges (gps_embedding.hip): the token / count words of a wave's range are requested in batches of 16 before
    the first use -- with a use next to each load the one-workgroup list builders walked their range one memory round
    trip at a time (33 us for 22 400 tokens).  No scratch: the hit masks and payloads stay in registers."""
    text = _asm("gps_embedding")
    for name, pat in (("dup_list_kernel", r"global_load_dword\s"), ("heavy_list_kernel", r"global_load_dwordx2"),
                      ("heavy_find_kernel", r"global_load_dword\s")):
        body, meta = _kernel(text, name)
        assert _meta(meta, "private_segment_fixed_size") == 0 and "scratch_" not in body, name
        runs = [len(re.findall(pat, seg)) for seg in re.split(r"s_waitcnt vmcnt", body)]
        assert max(runs) >= 12, (name, runs)


@pytest.mark.parametrize("which,max_vgpr", [("fwd", 128), ("bwd", 128)])
def test_fused_layernorm_issues_a_rows_loads_together(which, max_vgpr):
    # <float, unsigned short, 3>: fp32 residual stream, bf16 branch output, d = 768 -- the instantiation of the step
    body, meta = _kernel(_asm("gps_layernorm"), f"add_dropout_ln_{which}_kernelIftLi3E")
    assert _meta(meta, "private_segment_fixed_size") == 0 and "scratch_" not in body
    assert _meta(meta, "vgpr_count") <= max_vgpr                 # 4 waves per SIMD
    loop = body[body.index("s_cbranch_execz"):]                   # past the prologue (gamma / beta loads)
    runs = [len(re.findall(r"global_load_dwordx[24]", seg)) for seg in re.split(r"s_waitcnt vmcnt|s_cbranch", loop)]
    assert max(runs) >= (6 if which == "fwd" else 9), runs       # x, h (, dy) of all three 256-column steps in one batch


def test_grouped_weight_gradient_main_loop_has_no_waterfall_and_no_spill():
    body, meta = _kernel(_asm("gps_gemm"), "wgrad_grouped_kernel")
    assert _meta(meta, "vgpr_spill_count") == 0 and _meta(meta, "private_segment_fixed_size") == 0
    first, last = body.index("v_mfma"), body.rindex("v_mfma")
    loop = body[first:last]
    assert "v_readfirstlane" not in loop and "scratch_" not in loop
    # every LDS-DMA stage copy takes its descriptor from scalar registers: no exec-mask loop around it
    assert not re.search(r"s_and_saveexec_b64[^\n]*\n\s*buffer_load_dwordx4", loop)


def test_gemm_epilogues_have_no_ieee_division_sequences():
    """`__frcp_rn` / `1.f / x` compile to v_div_scale x2 + v_rcp + 4 v_fma + v_div_fmas + v_div_fixup per element -- a third of
    the GELU epilogue's vector instructions before round 4 replaced them by one v_rcp_f32."""
    text = _asm("gps_gemm")
    assert "v_div_scale_f32" not in text


def test_digest_is_reproducible_and_ignores_comments():
    """tools/asm_audit.py --digest: per kernel, a hash of the instructions and one of the .amdhsa_kernel descriptor.  Two
    compilations of a file agree, and so does a copy of the file with a comment line added (the `__hip_cuid_*` symbol,
    a hash of the source text, changes and must not count): the table moves only when the device code does."""
    import asm_audit
    src = os.path.join(ROOT, "sceneverse_amd", "csrc", "gps_embedding.hip")
    with tempfile.TemporaryDirectory() as tmp:
        first = asm_audit.digest(src, tmp)
        again = asm_audit.digest(src, tmp)
        copy_dir = os.path.join(tmp, "copy")
        os.mkdir(copy_dir)
        copy = os.path.join(copy_dir, "gps_embedding.hip")
        with open(src) as fh, open(copy, "w") as out:
            out.write("// a comment line that is not in the original\n" + fh.read())
        commented = asm_audit.digest(copy, tmp)
    names = [r[0] for r in first]
    assert any("sum_kernel" in n for n in names) and any("mark_kernel" in n for n in names) and names == sorted(names)
    for _, body, desc in first:
        assert len(body) == 64 and len(desc) == 64 and body != desc
    assert len({body for _, body, _ in first}) == len(first)       # different kernels, different instruction hashes
    assert first == again
    assert first == commented
