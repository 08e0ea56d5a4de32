"""Code-generation invariants of the decode projections' K loop, for every weight form (CPU: hipcc cross-compiles gfx950 here).

The load ring of dec_proj is inline assembly with exact vmcnt arithmetic, so inside the K loop the compiler must add no vmcnt waits of its
own and must not copy ring registers while their loads are in flight.  One trip of the loop is the whole ring, D 128-column groups: per
group WL non-temporal 16-byte weight loads (bf16 4, fp8 2, fp4 1), AL activation loads, a norm-weight load when the norm is folded in and,
for the code forms, one exponent dword; the code forms dequantise in registers, four v_cvt_scalef32_pk_bf16_fp8 / _fp4 per MFMA step."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
#        kernel                 weight loads per group, conversion, ring depth by AL
FORMS = {"bf16": ("dec_proj_kernel", 4, None, lambda al: 2),
         "fp8": ("dec_proj_f8_kernel", 2, "v_cvt_scalef32_pk_bf16_fp8", lambda al: 2),
         "fp4": ("dec_proj_f4_kernel", 1, "v_cvt_scalef32_pk_bf16_fp4", lambda al: 3 if al == 4 else 4)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("needs the ROCm clang")
    out = tmp_path_factory.mktemp("decode") / "decode.s"
    r = subprocess.run([CLANG, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-x", "hip",
                        os.path.join(ROOT, "audio-visual-llm_amd", "csrc", "decode.hip"), "--cuda-device-only", "-S", "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def _kernels(asm, stem):
    names = [n for n in re.findall(r"^(_Z\w+):", asm, flags=re.M) if stem + "IL" in n]
    return {n: asm.split("\n" + n + ":", 1)[1].split("s_endpgm")[0].split("\n") for n in names}


def _inner_loops(lines):
    """[(start, end)] of innermost loops: header comment .. the first scalar conditional branch."""
    out = []
    for i, l in enumerate(lines):
        if "Inner Loop Header" in l:
            j = next(k for k in range(i, len(lines)) if re.search(r"s_cbranch_scc[01]", lines[k]))
            out.append((i, j + 1))
    return out


def _ring_copies(body):
    """Instructions that move a ring register (or park it in an AGPR / scratch) inside the loop."""
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
    return bad


@pytest.mark.parametrize("form", list(FORMS))
def test_decode_k_loop_keeps_its_ring_without_compiler_waits(asm, form):
    stem, wl, cvt, depth = FORMS[form]
    kernels = _kernels(asm, stem)
    assert len(kernels) == 12                                     # NORM x 3 activation-load forms x adapters in the epilogue or not
    for name, lines in kernels.items():
        al = int(re.search(r"kernelILb[01]ELi(\d)E", name).group(1))
        norm = "kernelILb1E" in name
        d = depth(al)
        loops = _inner_loops(lines)
        assert len(loops) == 1, name                              # the K loop; the 1 .. 2D-1 groups left over are straight-line code
        a, b = loops[0]
        body = lines[a:b]
        assert sum("v_mfma_f32_16x16x32_bf16" in l for l in body) == 4 * d, name
        assert sum("v_cvt_scalef32_pk_bf16_fp" in l for l in body) == (16 * d if cvt else 0), name
        if cvt:
            assert sum(cvt in l for l in body) == 16 * d, name
        assert sum("global_load_dwordx4" in l for l in body) == d * (wl + al + norm), name
        assert sum(re.search(r"global_load_dwordx4 .*\bnt\b", l) is not None for l in body) == d * wl, name
        assert sum(re.search(r"global_load_dword\s", l) is not None for l in body) == (d if cvt else 0), name
        waits = [l.strip() for k, l in enumerate(body) if "s_waitcnt" in l and "vmcnt" in l and "ASMSTART" not in body[k - 1]]
        assert not waits, (name, waits)
        bad = _ring_copies(body)
        assert not bad, (name, bad[:4])
        assert not any("scratch_" in l for l in lines), name     # no scratch anywhere in the kernel either
    meta = {re.search(r"\.name:\s+(\S+)", blk).group(1): blk for blk in asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count")[1:]}
    meta = {k: v for k, v in meta.items() if stem + "IL" in k}
    assert len(meta) == 12
    for k, blk in meta.items():
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) == 0, k
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, k
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 128, k      # two workgroups of 8 waves per CU
