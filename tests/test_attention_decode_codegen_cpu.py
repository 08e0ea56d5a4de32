"""Resources of the single-token attention kernel (csrc/attention_decode.hip), for every row form and wave count (CPU: hipcc cross-compiles
gfx950 here).

One kernel body serves the plain f32 and bf16 rows and the e4m3 image, at 4 and at 16 waves.  A 1024-thread workgroup has 128 VGPRs per lane and
the e4m3 form is close to that, so a row form that holds more in flight would spill: no instantiation may spill or use scratch, and each has
the LDS of its merge buffers alone ((128 + 2) floats per wave).  Read from the code object's metadata only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ROWS = {"f32": "8PlainRowIfEE", "bf16": "8PlainRowIDF16bEE", "e4m3": "7E4m3RowE"}       # the row form as the kernel's mangled name spells it


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("needs the ROCm clang")
    out = tmp_path_factory.mktemp("attention_decode") / "attention_decode.s"
    r = subprocess.run([CLANG, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                        os.path.join(ROOT, "audio-visual-llm_amd", "csrc", "attention_decode.hip"), "--cuda-device-only", "-S", "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = out.read_text()
    return {re.search(r"\.name:\s+(\S+)", blk).group(1): blk for blk in asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count")[1:]}


def test_six_kernels_without_spills_or_scratch(meta):
    assert len(meta) == 6, sorted(meta)
    want = {f"attn_decode1_kernelINS_{row}Li{nw}E": nw for row in ROWS.values() for nw in (4, 16)}
    for stem, nw in want.items():
        names = [k for k in meta if stem in k]
        assert len(names) == 1, (stem, sorted(meta))
        blk = meta[names[0]]
        val = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))  # noqa: E731
        assert val("vgpr_spill_count") == 0, names[0]
        assert val("private_segment_fixed_size") == 0, names[0]
        assert val("vgpr_count") <= 128, (names[0], val("vgpr_count"))         # 1024 threads: 16 waves on 4 SIMDs of 512 registers per lane
        assert val("group_segment_fixed_size") == nw * (128 + 2) * 4, names[0]   # 8320 at 16 waves, 2080 at 4
