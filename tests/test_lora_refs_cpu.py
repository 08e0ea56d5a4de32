"""CPU: the float64 restatements of tests/refs64_lora.py against plain torch float64 matmul and keep_grid masking, the host emulation of the
documented arithmetic UNDER every bar of tests/bars.py ("LoRA adapter kernels against float64") at every family x geometry that
tests/test_lora_pin_gpu.py runs, the zero-bar families' condition on the reference alone, each mutant of the emulation OVER a bar in at least one
family, and the seed wrap of av_seed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refs64_gemm as G  # noqa: E402
import refs64_lora as RL  # noqa: E402

F64 = torch.float64


def close(a, b):
    return float((a - b).abs().max()) < 1e-12 * max(1.0, float(b.abs().max()))


def test_rank3_64_is_torch_matmul():
    A, _ = RL._ab("randn", 19, 256, 0)
    Bs = [RL.pad_rows(RL._ab("randn", 19, 256, j)[1], 8) for j in range(3)]
    seeds = list(RL.SEEDS)
    for j, ref in enumerate(RL.rank3([A], Bs, 8, 0.5, seeds, 0.05, shared=True)):
        k = G.keep_grid(seeds[j], 19, 256, 256, 0.05)
        xd = torch.where(k, (A.double() * G.drop_scale(0.05)).float().bfloat16().double(), torch.zeros(19, 256, dtype=F64))
        assert close(ref.out[:, :8], 0.5 * xd @ Bs[j].double()[:8].t()) and bool((ref.out[:, 8:] == 0).all()) and ref.out.shape == (19, 64)
        assert close(ref.sum_abs[:, :8], xd.abs() @ Bs[j].double()[:8].abs().t()) and bool((ref.sum_abs[:, 8:] == 0).all())
    As = [RL._ab("randn", 19, K, j)[0] for j, K in enumerate(RL.RK_SPLIT_K)]
    Bs = [RL._ab("randn", 19, K, j)[1] for j, K in enumerate(RL.RK_SPLIT_K)]
    for j, ref in enumerate(RL.rank3(As, Bs, 16, 2.0, seeds, 0.0, shared=False)):
        assert close(ref.out[:, :16], 2.0 * As[j].double() @ Bs[j].double().t()) and bool((ref.out[:, 16:] == 0).all())


def test_tn_multi64_is_torch_matmul():
    big, q, o = G.family_tn("randn", 70, 256, 48)
    sm = [q[:, 16 * j:16 * j + 16] for j in range(3)]
    seeds = list(RL.SEEDS)
    o0 = [o[:, 16 * j:16 * j + 8].t().contiguous() for j in range(3)]
    for j, ref in enumerate(RL.tn_multi(big, sm, 8, o0, 0.5, seeds, 0.05, shared=True)):
        k = G.keep_grid(seeds[j], 70, 256, 256, 0.05)
        xd = torch.where(k, (big.double() * G.drop_scale(0.05)).float().bfloat16().double(), torch.zeros(70, 256, dtype=F64))
        assert ref.out.shape == (8, 256) and close(ref.out, o0[j].double() + 0.5 * sm[j].double()[:, :8].t() @ xd)
    cols = [(0, 128), (128, 128)]
    o0 = [o[c0:c0 + nc, 16 * j:16 * j + 8].contiguous() for j, (c0, nc) in enumerate(cols)]
    for j, ref in enumerate(RL.tn_multi(big, sm[:2], 8, o0, 2.0, shared=False, cols=cols)):
        assert ref.out.shape == (128, 8) and close(ref.out, o0[j].double() + 2.0 * big.double()[:, 128 * j:128 * j + 128].t() @ sm[j].double()[:, :8])


def test_dx_masked64_is_torch_matmul():
    Ts, ATs, R = RL.family_dx("randn", 37, 128, 16, 3)
    seeds = list(RL.SEEDS)
    ref = RL.dx_masked(Ts, ATs, seeds, 16, 0.05, R)
    want = R.double()
    for j in range(3):
        k = G.keep_grid(seeds[j], 37, 128, 128, 0.05).double()
        want = want + k * G.drop_scale(0.05) * (Ts[j].double() @ ATs[j].double().t())
    assert close(ref.out, want)
    assert close(RL.dx_masked(Ts, ATs, seeds, 4, 0.0).out, sum(Ts[j].double()[:, :4] @ ATs[j].double()[:, :4].t() for j in range(3)))


def test_seed_wraps_at_2_32():
    """The effective seed is (base + offset) mod 2^32: a base that carries the sum past 2^32 gives the wrapped seed's mask, not the offset's."""
    assert all(RL.WRAP_BASE + s >= 2 ** 32 for s in RL.SEEDS)
    assert RL.eff_seed(RL.WRAP_BASE, RL.SEEDS[0]) == RL.SEEDS[0] - 0x100 and RL.eff_seed(0xFFFFFFFF, 1) == 0
    Ts, ATs, _ = RL.family_dx("randn", 33, 128, 16, 1)
    ref = RL.dx_masked(Ts, ATs, [RL.SEEDS[0]], 16, 0.5, base=RL.WRAP_BASE)
    assert torch.equal(ref.keeps[0], G.keep_grid(RL.SEEDS[0] - 0x100, 33, 128, 128, 0.5))
    assert not torch.equal(ref.keeps[0], G.keep_grid(RL.SEEDS[0], 33, 128, 128, 0.5))


# ------------------------------------------------------------------------------------------------ the emulation under the bars, the mutants over one
def run(c, mut=None):
    bufs, _ = RL.images(c)
    return RL.check(c, RL.emul(c, bufs, mut))


def sweep(cases):
    worst, n = 0.0, 0
    for c, what in cases:
        if c["fam"] in G.ZERO_BAR:
            assert RL.zero_bar_ok(c), f"{what}: the float64 result is not representable in the output format"
        canary, over, ratio = run(c)
        assert canary == 0 and over == 0, (what, canary, over, ratio)
        worst, n = max(worst, ratio), n + 1
    assert worst < 1.0
    return n, worst


@pytest.mark.parametrize("M", RL.RK_M)
def test_emulation_under_every_bar_rank3(M):
    print("RATIO emul rank3 M=%d: %d cases, worst %.3f" % ((M,) + sweep(RL.cases_rank3(M))))


@pytest.mark.parametrize("M", RL.TN_M)
def test_emulation_under_every_bar_tn_multi(M):
    print("RATIO emul tn_multi M=%d: %d cases, worst %.3f" % ((M,) + sweep(RL.cases_tn(M))))
    if M in RL.TN_GUARD_M:
        sweep(RL.cases_tn_guard(M))


@pytest.mark.parametrize("M", RL.DX_M)
def test_emulation_under_every_bar_dx_masked(M):
    print("RATIO emul lora_dx M=%d: %d cases, worst %.3f" % ((M,) + sweep(RL.cases_dx(M))))


def test_tables_take_every_value_of_every_axis():
    """What the issue lists per axis is in the tables (a table edited later cannot silently lose a value)."""
    col = lambda t, i: {r[i] for r in t}
    assert col(RL.RK_SHARED, 0) == {256, 512, 1024, 1280} and col(RL.RK_SHARED, 1) == {1, 2, 3} and col(RL.RK_SHARED, 2) == {1, 8, 16}
    assert col(RL.RK_SHARED, 3) == {0.0, "p"} and col(RL.RK_SHARED, 4) == {2.0, 0.5} and col(RL.RK_SHARED, 5) == {"one", "sep"}
    assert RL.WRAP_BASE in col(RL.RK_SHARED, 6) and col(RL.RK_SPLIT, 0) == {1, 2, 3} and RL.RK_SPLIT_K == (1280, 256, 512)
    assert col(RL.TN_SHARED, 0) == {128, 384} and col(RL.TN_SHARED, 1) == {1, 2, 3} and col(RL.TN_SHARED, 2) == {1, 8, 16}
    assert col(RL.TN_SHARED, 3) == {0.0, "p"} and col(RL.TN_SHARED, 4) == {1.0, 0.5} and RL.WRAP_BASE in col(RL.TN_SHARED, 5)
    assert col(RL.TN_SPLIT, 0) == {(128,), (128, 128), (256, 128, 128), (128, 256, 128)} and col(RL.TN_SPLIT, 1) == {1, 8, 16}
    assert col(RL.TN_SPLIT, 2) == {1.0, 0.5}
    assert col(RL.DX, 0) == {128, 384} and col(RL.DX, 1) == {1, 2, 3} and col(RL.DX, 2) == {4, 16, 32} and col(RL.DX, 3) == {0.0, "p"}
    assert col(RL.DX, 4) == {32, 64, "slice"} and col(RL.DX, 5) == {"none", "sep", "alias"} and RL.WRAP_BASE in col(RL.DX, 6)
    assert {G.drop_p(f) for f in G.FAMILIES} == {0.05, 0.5}
    assert RL.RK_M == (1, 15, 16, 17, 50) and RL.TN_M == (1, 63, 64, 65, 300, 700, 8300) and RL.DX_M == (1, 31, 32, 33, 127, 128, 129, 200)
    # the chunk split of gemm_tn_multi at the edge M: one chunk, several with a ragged last one, and the 32-chunk cap
    assert RL.tn_chunks(65, 256) == (1, 128) and RL.tn_chunks(300, 256) == (2, 192) and RL.tn_chunks(700, 256) == (3, 256)
    assert RL.tn_chunks(8300, 256) == (26, 320) and -(-8300 // 256) > 32 and RL.tn_chunks(8300, 512) == (17, 512)


# mutant -> the cases it is tried on: (builder, arguments).  Each is a geometry in which the mutated term exists.
# (mask_stride has no rank3 case: avllm_lora_rank3 refuses a masked A whose row stride is not K.)
MUTANT_CASES = {
    "seed0_all": [(RL.case_rank3, (17, RL.RK_SHARED[2], True)), (RL.case_tn, (65, RL.TN_SHARED[2], True)), (RL.case_dx, (33, RL.DX[1]))],
    "mask_stride": [(RL.case_tn, (65, RL.TN_SHARED[1], True)), (RL.case_dx, (33, RL.DX[1]))],
    "no_scale": [(RL.case_rank3, (17, RL.RK_SHARED[1], True)), (RL.case_tn, (65, RL.TN_SHARED[1], True)), (RL.case_dx, (33, RL.DX[1]))],
    "pad_unwritten": [(RL.case_rank3, (17, RL.RK_SHARED[1], True)), (RL.case_rank3, (17, RL.RK_SPLIT[2], False))],
    "slab_tail": [(RL.case_tn, (65, RL.TN_SHARED[0], True)), (RL.case_tn, (300, RL.TN_SPLIT[1], False))],
    "range_neighbour": [(RL.case_tn, (65, RL.TN_SPLIT[1], False)), (RL.case_tn, (65, RL.TN_SPLIT[3], False))],
    "rows_ge_R": [(lambda fam, M, row, sh: RL.case_tn(fam, M, row, sh, padded=False, sentinel=RL.SENTINEL), (65,) + RL.TN_GUARD[0][::-1]),
                  (lambda fam, M, row, sh: RL.case_tn(fam, M, row, sh, padded=False, sentinel=RL.SENTINEL), (65,) + RL.TN_GUARD[1][::-1])],
    "round_per_adapter": [(RL.case_dx, (33, RL.DX[1])), (RL.case_dx, (33, RL.DX[2]))],
    "mask_after_R": [(RL.case_dx, (33, RL.DX[1])), (RL.case_dx, (33, RL.DX[2]))],
    "seed_dev_ignored": [(RL.case_rank3, (17, RL.RK_SHARED[3], True)), (RL.case_tn, (65, RL.TN_SHARED[4], True)), (RL.case_dx, (33, RL.DX[3]))],
}


@pytest.mark.parametrize("mut", RL.MUTANTS)
def test_mutant_exceeds_a_bar(mut):
    """Every listed case must catch the mutant in at least one family while the unmutated emulation passes the very same case."""
    for build, args in MUTANT_CASES[mut]:
        caught = []
        for fam in G.FAMILIES:
            c = build(fam, *args)
            assert run(c)[:2] == (0, 0), (mut, c["kind"], fam)
            canary, over, _ = run(c, mut)
            if canary or over:
                caught.append((fam, canary, over))
        print(f"MUTANT {mut} {c['kind']} {args}: {caught}")
        assert caught, f"{mut} on {c['kind']} {args}: under every bar in every family"
        if mut == "round_per_adapter":
            assert "offset" in [x[0] for x in caught]                      # the header's "rounded once"


def test_rows_ge_R_needs_the_guard_case():
    """Why the guard cases exist: with the padded Small of the main table (zeros past R) the rows >= R of the product are exact zeros, and a float
    atomic onto a NaN border leaves NaN: the mutant is invisible there, in every family."""
    for fam in G.FAMILIES:
        assert run(RL.case_tn(fam, 65, RL.TN_GUARD[0][1], True), "rows_ge_R")[:2] == (0, 0)
