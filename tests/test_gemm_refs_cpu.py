"""CPU: the float64 GEMM restatements of tests/refs64_gemm.py against torch's float64 linear / gelu, the numpy dropout mask against a host program
compiled from csrc/common.h, the host emulation of the documented arithmetic UNDER every bar of tests/bars.py ("GEMM against float64") at every
family x geometry of tests/test_gemm_pin_gpu.py, and each mutant of the emulation OVER a bar in at least one family."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bars as Bar  # noqa: E402
import refs64_gemm as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
R0, C0 = 1, 8            # where C starts inside the NaN buffer


def test_gemm64_is_torch_linear():
    d = G.family("randn", 37, 24, 128, 64)
    bias, R = d["bias"], d["R"][:5]
    for act, fn in ((G.ACT_NONE, lambda x: x), (G.ACT_GELU, torch.nn.functional.gelu), (G.ACT_SILU, torch.nn.functional.silu),
                    (G.ACT_QUICK_GELU, lambda x: x * torch.sigmoid(1.702 * x))):
        r = G.gemm(d["A"], d["B"], d["A2"], d["B2"], bias=bias, R=R, act=act, alpha=0.5, r_mod=5, remap=(13, 14, 1))
        lin = torch.nn.functional.linear(torch.cat([d["A"], d["A2"]], 1).double(), torch.cat([d["B"], d["B2"]], 1).double())
        want = fn(0.5 * lin + bias.double()) + R.double()[torch.arange(37) % 5]
        assert float((r.out - want).abs().max()) < 1e-12
        assert torch.equal(r.rows, torch.tensor([(m // 13) * 14 + 1 + m % 13 for m in range(37)]))
    r = G.gemm(d["A"], d["B"], n_valid=8)
    assert float((r.out[:, :16] - d["A"].double() @ d["B"].double().t()[:, :16]).abs().max()) < 1e-12 and bool((r.out[:, 16:] == 0).all())
    assert float((r.sum_abs[:, :16] - d["A"].double().abs() @ d["B"].double().abs().t()[:, :16]).abs().max()) < 1e-12


def test_gemm_tn64_is_torch():
    p, q, o = G.family_tn("randn", 70, 128, 16)
    r = G.gemm_tn(p, q, J=8, alpha=2.0, out=o[:, :8])
    want = o[:, :8].double() + 2.0 * torch.nn.functional.linear(p.double().t(), q.double()[:, :8].t())
    assert float((r.out - want).abs().max()) < 1e-12


def test_mask_is_pure_scaling():
    d = G.family("randn", 9, 16, 64)
    r0 = G.gemm(d["A"], d["B"])
    r = G.gemm(d["A"], d["B"], drop=(7, 0.5))
    k = G.keep_grid(7, 9, 16, 16, 0.5)
    assert torch.equal(r.out, torch.where(k, 2.0 * r0.out, torch.zeros_like(r0.out))) and 0.3 < float(k.double().mean()) < 0.7
    assert G.drop_thr(0.05) == 3276 and abs(G.drop_scale(0.05) - 65536.0 / (65536 - 3276)) < 1e-7 and G.drop_scale(0.5) == 2.0


KEEP_PROG = r'''
#include "common.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
    const uint32_t seed = (uint32_t)strtoul(argv[1], nullptr, 0);
    const float p = (float)atof(argv[2]);
    for (int i = 3; i < argc; ++i) {
        const unsigned long long i0 = strtoull(argv[i], nullptr, 0);
        for (unsigned long long j = 0; j < 64; ++j) putchar(av_keep(seed, i0 + j, p) ? '1' : '0');
    }
    printf("\n%u %.9g\n", av_drop_thr(p), (double)av_drop_scale(p));
    return 0;
}
'''


def test_keep_is_common_h_bit_for_bit(tmp_path):
    """av_keep / av_drop_thr / av_drop_scale are __host__ __device__: a tiny host main compiled from csrc/common.h is the yardstick."""
    src = tmp_path / "keep.hip"
    src.write_text(KEEP_PROG)
    exe = str(tmp_path / "keep")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "audio-visual-llm_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    starts = [0, 1000, 2 ** 32 - 32, 2 ** 33 - 32, 2 ** 33 + 1, 2 ** 34 + 12345, 3 * 2 ** 33 - 7, 2 ** 40 + 3]
    for seed in (0, 1, 0x5EED1234, 0xFFFFFFFF):
        for p in (0.05, 0.5, 1.0 / 65536):
            out = subprocess.check_output([exe, str(seed), repr(p)] + [str(s) for s in starts]).decode().split("\n")
            want = np.array([c == "1" for c in out[0]])
            idx = np.concatenate([np.arange(64, dtype=np.uint64) + np.uint64(s) for s in starts])
            got = G.keep(seed, idx, p)
            assert np.array_equal(got, want), (seed, p, int((got != want).sum()))
            thr, sc = out[1].split()
            assert int(thr) == G.drop_thr(p) and float(sc) == pytest.approx(G.drop_scale(p), rel=1e-8, abs=0)


# ------------------------------------------------------------------------------------------------ the emulation under the bars, the mutants over one
def run_case(fam, M, N, K, K2, e, kind="mfma", mut=None, f32_in=False, rows=None):
    """One avllm_gemm case on the host: the float64 reference, its bar, the emulation's buffer -> (canaries, over, ratio).  rows: a row subset
    (the emulation of a subset of rows is the same arithmetic)."""
    r_rows = e.r_mod if e.r_mod else M
    d = G.family(fam, M, N, K, K2, r_rows=r_rows)
    if rows is not None:
        d["A"], d["R"] = d["A"][rows], d["R"][rows] if not e.r_mod else d["R"]
        d["A2"] = None if d["A2"] is None else d["A2"][rows]
        M = len(rows)
    bias = d["bias"] if e.bias else None
    drop = (G.DROP_SEED, G.drop_p(fam)) if e.drop else None
    R = d["R"] if e.R else None
    if fam == "offset" and e.R and not e.r_mod:
        R = G.cancel_R(G.gemm(d["A"], d["B"], d["A2"], d["B2"], bias=bias, act=e.act, alpha=e.alpha, drop=drop).out, r_rows)
    ref = G.gemm(d["A"], d["B"], d["A2"], d["B2"], bias=bias, R=R, act=e.act, alpha=e.alpha, r_mod=e.r_mod, remap=e.remap, drop=drop)
    out_bf16 = not (e.f32 or f32_in)
    if fam == "exact":
        assert G.exact_holds(ref), (M, N, K, K2, e.name)
    bar = 0.0 if fam in G.ZERO_BAR else Bar.gemm_bar(ref, K + K2, kind, e.act, e.alpha, out_bf16)
    total_rows = int(ref.rows.max()) + 1 + R0 + 3
    buf = torch.full((total_rows, (N + 3) // 4 * 4 + 16), float("nan"), dtype=F64)
    if e.inplace:
        buf[R0:R0 + M, C0:C0 + N] = R.double()
    G.emul(buf, R0, C0, d["A"], d["B"], d["A2"], d["B2"], bias=bias, R=None if e.inplace else R, act=e.act, alpha=e.alpha, r_mod=e.r_mod,
           remap=e.remap, drop=drop, out_bf16=out_bf16, inplace=e.inplace, mut=mut)
    return G.verify(buf, R0, C0, ref.rows, N, ref.out, bar)


@pytest.mark.parametrize("MN", G.TILE_MN, ids=lambda mn: f"{mn[0]}x{mn[1]}")
def test_emulation_under_every_bar_tiled(MN):
    M, N = MN
    worst = 0.0
    for K, K2 in G.TILE_K:
        for fam in G.FAMILIES:
            for e in G.EPIS:
                if not G.epi_ok(fam, e):
                    continue
                canary, over, ratio = run_case(fam, M, N, K, K2, e)
                assert canary == 0 and over == 0, (fam, K, K2, e.name, canary, over, ratio)
                worst = max(worst, ratio)
    print(f"RATIO emul tiled {M}x{N} {worst:.3f}")
    assert worst < 1.0


def test_emulation_under_every_bar_persistent_rows():
    for M, N in ((17 * 256 - 3, 16 * 256 - 8), (34 * 256 - 3, 16 * 128 - 8)):
        rows = G.sample_rows(M)
        for K in G.PERSIST_K:
            for fam in G.FAMILIES:
                for e in (G.EPIS[0], G.EPIS[3], G.EPIS[7]):
                    if G.epi_ok(fam, e):
                        canary, over, ratio = run_case(fam, M, N, K, 0, e, rows=rows)
                        assert canary == 0 and over == 0, (M, N, K, fam, e.name, over, ratio)


def test_emulation_under_every_bar_smallm_skinny_f32():
    for M in G.SMALLM_M:
        for N in G.SMALLM_N:
            for K in G.SMALLM_K:
                for K2 in G.SMALLM_K2:
                    for fam in G.FAMILIES:
                        for e in G.SMALLM_EPIS:
                            if G.epi_ok(fam, e):
                                assert run_case(fam, M, N, K, K2, e, kind="split8")[:2] == (0, 0), (M, N, K, K2, fam, e.name)
    for M, N in G.F32_MN:
        for K in G.F32_K:
            for K2 in G.F32_K2:
                for fam in G.FAMILIES:
                    for e in G.F32_EPIS:
                        if G.epi_ok(fam, e):
                            assert run_case(fam, M, N, K, K2, e, kind="f32", f32_in=True)[:2] == (0, 0), (M, N, K, K2, fam, e.name)
    for M in G.SKINNY_M:
        for K in G.SKINNY_K:
            for nv in G.SKINNY_NV:
                for fam in G.FAMILIES:
                    d = G.family(fam, M, 64, K)
                    if nv > 0:
                        d["B"][nv:] = 0                         # the caller's side of n_valid: rows [n_valid, 64) of B are zero
                    a_drop = (G.DROP_SEED, G.drop_p(fam))
                    ref = G.gemm(d["A"], d["B"], alpha=0.5, a_drop=a_drop, n_valid=nv)
                    if fam == "exact":
                        assert G.exact_holds(ref)
                    bar = 0.0 if fam in G.ZERO_BAR else Bar.gemm_bar(ref, K, "split8", 0, 0.5, True)
                    buf = torch.full((M + R0 + 3, 80), float("nan"), dtype=F64)
                    G.emul(buf, R0, C0, d["A"], d["B"], alpha=0.5, a_drop=a_drop, n_valid=nv)
                    assert G.verify(buf, R0, C0, ref.rows, 64, ref.out, bar)[:2] == (0, 0), (M, K, nv, fam)


def test_exact_family_is_exact_at_every_k():
    """The exact family's condition (float64 result representable in bf16) at every reduction length the GPU file uses, up to 4096 + 64, with the
    widest epilogue (alpha in {1, 0.5}, bias, R) and with the p = 0.5 mask."""
    for K, K2 in G.TILE_K + ((2304, 0), (2304, 64), (4096, 64), (320, 0)):
        d = G.family("exact", 67, 72, K, K2)
        for alpha in (1.0, 0.5):
            assert G.exact_holds(G.gemm(d["A"], d["B"], d["A2"], d["B2"], bias=d["bias"], R=d["R"], alpha=alpha, drop=(3, 0.5)))
            assert G.exact_holds(G.gemm(d["A"], d["B"], d["A2"], d["B2"], bias=d["bias"], R=d["R"], alpha=alpha))
    d = G.family("exact", 300, 64, 2304)
    assert G.exact_holds(G.gemm(d["A"], d["B"], alpha=0.5, a_drop=(3, 0.5)))


def test_emulation_under_tn_bar():
    for M in G.TN_M:
        for I in G.TN_I + (272,):
            for J in G.TN_J + (17,):
                for fam in G.FAMILIES:
                    mfma = I % 128 == 0 and J <= 16
                    p, q, o = G.family_tn(fam, M, I, J)
                    drop = (G.DROP_SEED, G.drop_p(fam)) if mfma else None
                    ref = G.gemm_tn(p, q, alpha=0.5, drop=drop, out=o)
                    got = G.emul_tn(p, q, I, J, 0.5, drop, o)
                    if fam in G.ZERO_BAR:
                        assert torch.equal(got, ref.out), (M, I, J, fam)
                        assert torch.equal(ref.out, ref.out.float().double())
                    else:
                        assert bool(((got - ref.out).abs() <= Bar.gemm_tn_bar(ref, M, 0.5, o.double(), mfma)).all()), (M, I, J, fam)


MUTANT_CASES = {                    # mutant -> (K, K2, epilogue name): a geometry and an epilogue in which the mutated term exists
    "drop_kstep": (192, 64, "plain"), "k2_twice": (192, 64, "bias"), "bias_shift": (128, 0, "bias"), "r_row": (128, 0, "rmod_remap"),
    "subtile_T": (128, 0, "plain"), "edge_clamp": (128, 0, "bias_R"), "mask_ldc": (128, 0, "drop"), "round_before_R": (128, 0, "R"),
    "alpha_after_bias": (128, 0, "alpha"),
}


@pytest.mark.parametrize("mut", G.MUTANTS)
def test_mutant_exceeds_a_bar(mut):
    K, K2, name = MUTANT_CASES[mut]
    e = next(x for x in G.EPIS if x.name == name)
    caught = []
    for fam in G.FAMILIES:
        canary, over, ratio = run_case(fam, 129, 136, K, K2, e, mut=mut)
        if canary or over:
            caught.append((fam, canary, over))
        assert run_case(fam, 129, 136, K, K2, e)[:2] == (0, 0)          # and the unmutated emulation passes the very same case
    print(f"MUTANT {mut}: {caught}")
    assert caught, f"{mut}: under every bar in every family"
    if mut == "round_before_R":
        assert "offset" in [c[0] for c in caught]                      # the single-rounding statement
