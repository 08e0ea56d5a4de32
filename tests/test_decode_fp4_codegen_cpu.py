"""Code-generation invariants of the fp4 weight form of the decode projections (CPU: hipcc cross-compiles gfx950 here).

The same standard as the bf16 and fp8 forms (test_codegen_cpu.py, test_decode_fp8_codegen_cpu.py): the load ring is inline assembly with exact
vmcnt arithmetic, so the compiler must add no vmcnt waits of its own inside the K loop and must not copy ring registers while their loads are
in flight.  On top of that the loop must dequantise in registers -- four v_cvt_scalef32_pk_bf16_fp4 per 32-wide MFMA step -- and stream one
16-byte (non-temporal) code load per four MFMA steps, a quarter of the bf16 form's weight loads."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _asm(src, tmp_path):
    out = tmp_path / (os.path.basename(src) + ".s")
    r = subprocess.run([CLANG, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-x", "hip", src,
                        "--cuda-device-only", "-S", "-o", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def _kernels(asm, pattern):
    names = [n for n in re.findall(r"^(_Z\w+):", asm, flags=re.M) if re.search(pattern, n)]
    return {n: asm.split("\n" + n + ":", 1)[1].split("s_endpgm")[0].split("\n") for n in names}


def _inner_loops(lines):
    out = []
    for i, l in enumerate(lines):
        if "Inner Loop Header" in l:
            j = next(k for k in range(i, len(lines)) if re.search(r"s_cbranch_scc[01]", lines[k]))
            out.append((i, j + 1))
    return out


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs the ROCm clang")
def test_decode_fp4_ring_dequantises_in_registers_without_compiler_waits(tmp_path):
    asm = _asm(os.path.join(ROOT, "audio-visual-llm_amd", "csrc", "decode.hip"), tmp_path)
    kernels = _kernels(asm, r"dec_proj_f4_kernel")
    assert len(kernels) == 12                                     # NORM x 3 activation-load forms x adapters in the epilogue or not
    for name, lines in kernels.items():
        al = int(re.search(r"f4_kernelILb[01]ELi(\d)E", name).group(1))
        norm = "f4_kernelILb1E" in name
        loops = _inner_loops(lines)
        assert len(loops) == 1, name                              # the K loop; the 1 .. 2D-1 groups left over are straight-line code
        a, b = loops[0]
        body = lines[a:b]
        mfma = sum("v_mfma_f32_16x16x32_bf16" in l for l in body)
        assert mfma > 0 and mfma % 4 == 0, name
        groups = mfma // 4                                        # one trip = the whole ring: D 128-column groups
        assert groups == (3 if al == 4 else 4), name
        assert sum("v_cvt_scalef32_pk_bf16_fp4" in l for l in body) == 4 * mfma, name
        # per group: 1 non-temporal code load, AL activation loads (+ 1 norm-weight load), 1 exponent dword
        assert sum(re.search(r"global_load_dwordx4 .*\bnt\b", l) is not None for l in body) == groups, name
        assert sum("global_load_dwordx4" in l for l in body) == groups * (1 + al + norm), name
        assert sum(re.search(r"global_load_dword\s", l) is not None for l in body) == groups, name
        waits = [l.strip() for k, l in enumerate(body) if "s_waitcnt" in l and "vmcnt" in l and "ASMSTART" not in body[k - 1]]
        assert not waits, (name, waits)
        bad = []
        for k, l in enumerate(body):
            if re.search(r"scratch_|v_accvgpr", l):
                bad.append(l.strip())
            m = re.search(r"v_mov_b32_e32 (v\d+), v\d+", l)
            if m:       # benign only as the `old` operand of the DPP move that follows (row rotate / broadcast of an operand AFTER its wait)
                nxt = next((x for x in body[k + 1:k + 80] if re.search(r"\b" + m.group(1) + r"\b", x)), "")
                if "_dpp" not in nxt or not re.search(r"v_mov_b32_dpp " + m.group(1) + r",", nxt):
                    bad.append(l.strip())
            if re.search(r"v_mov_b64_e32 v\[\d+:\d+\], v\[", l):
                bad.append(l.strip())
        assert not bad, (name, bad[:4])
        assert not any("scratch_" in l for l in lines), name     # no scratch anywhere in the kernel either
    meta = {re.search(r"\.name:\s+(\S+)", blk).group(1): blk for blk in asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count")[1:]}
    f4 = {k: v for k, v in meta.items() if "dec_proj_f4_kernel" in k}
    assert len(f4) == 12
    for k, blk in f4.items():
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, k
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, k
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 128, k      # two workgroups of 8 waves per CU
