"""Resources of the shared-prefix attention kernels (csrc/attention_decode_shared.hip), for every row form, query count and launch form (CPU:
hipcc cross-compiles gfx950 here), by the method of test_attention_decode_codegen_cpu.py.

The prefix kernels and the two-launch output kernel run 256-thread workgroups: one wave per SIMD, so a lane may hold up to 512 registers, but
the launches are sized for several workgroups per CU (their bytes in flight come from them): the budget here is 256 VGPRs, two workgroups per
CU at the worst (the 4-query e4m3 form holds 4 x (16 q + 16 acc) floats besides the rows in flight), and the 1- and 2-query forms and the
output kernel stay within 168 (three).  The one-launch output kernel is a 1024-thread workgroup as attn_decode1_kernel's: 128 VGPRs.  No
instantiation may spill or use scratch, and each has the LDS of its merge buffers alone: (128 + 2) floats per wave and query.  Read from the
code object's metadata only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ROWS = {"bf16": "8PlainRowIDF16bEE", "e4m3": "7E4m3RowE"}       # the row form as the kernel's mangled name spells it


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("needs the ROCm clang")
    out = tmp_path_factory.mktemp("attention_decode_shared") / "attention_decode_shared.s"
    r = subprocess.run([CLANG, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                        os.path.join(ROOT, "audio-visual-llm_amd", "csrc", "attention_decode_shared.hip"), "--cuda-device-only", "-S", "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    return {re.search(r"\.name:\s+(\S+)", blk).group(1): blk for blk in asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count")[1:]}


def test_ten_kernels_without_spills_or_scratch(meta):
    assert len(meta) == 10, sorted(meta)
    # stem -> (waves, queries per pass, VGPR budget)
    want = {f"attn_shared_prefix_kernelINS_{row}Li{qc}E": (4, qc, 256 if qc == 4 else 168) for row in ROWS.values() for qc in (1, 2, 4)}
    want.update({f"attn_shared_out_kernelINS_{row}Li4ELb0E": (4, 1, 168) for row in ROWS.values()})
    want.update({f"attn_shared_out_kernelINS_{row}Li16ELb1E": (16, 1, 128) for row in ROWS.values()})
    for stem, (nw, qc, budget) in want.items():
        names = [k for k in meta if stem in k]
        assert len(names) == 1, (stem, sorted(meta))
        blk = meta[names[0]]
        val = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))  # noqa: E731
        assert val("vgpr_spill_count") == 0, names[0]
        assert val("sgpr_spill_count") == 0, names[0]
        assert val("private_segment_fixed_size") == 0, names[0]
        assert val("max_flat_workgroup_size") == nw * 64, names[0]
        assert val("vgpr_count") <= budget, (names[0], val("vgpr_count"))
        assert val("group_segment_fixed_size") == nw * qc * (128 + 2) * 4, names[0]      # 2080 per query at 4 waves, 8320 at 16
