"""CPU checks of tests/refs64_fp8.py: a mistake there must not become the yardstick of tests/test_fp8_pin_gpu.py.  decode() against the oracle and
torch's own e4m3; the host scale image against the index arithmetic of csrc/fp8.hip's header, written out as loops; the premise of every zero-bar
family (exact partial sums, results representable in the output format, the engineered power-of-two and saturating blocks); the quantised-output
rules on the rule's own output; and the size of the set of codes and exponents the norm's fp32 bar leaves undetermined."""
import pytest
import torch

import bars as Bar
import refs64_fp8 as F8
import refs64_gemm as G
from oracle import mxfp8 as MX

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def test_decode_is_the_e4m3_table_times_the_scale():
    codes = torch.arange(256, dtype=torch.uint8).reshape(8, 32)
    exps = torch.tensor([[-127], [-9], [-1], [0], [1], [8], [100], [119]], dtype=torch.int32)
    got = F8.decode(codes, exps)
    t = codes.view(torch.float8_e4m3fn).double()
    nan = torch.isnan(t)
    assert int(nan.sum()) == 2 and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan], (t * F8.pow2(exps))[~nan])
    ok = (exps > -127).expand(8, 32) & ~nan                              # the oracle forms 2^e in fp32, exact above the denormal range
    assert torch.equal(got[ok], MX.dequantize(codes, exps).double()[ok])
    vals = torch.tensor([0.0, 2.0 ** -9, 0.015625, 1.0, 1.125, 15.0, 448.0, -448.0, -3.0])
    assert torch.equal(F8.E4M3[F8.code_of(vals).long()], vals.double())


@pytest.mark.parametrize("K", (128, 384))
@pytest.mark.parametrize("R", (1, 17, 65, 257, 300))
@pytest.mark.parametrize("layout", (0, 1, 2))
def test_scale_image_round_trip_and_header_arithmetic(layout, R, K):
    exps = torch.randint(-126, 128, (R, K // 32), generator=torch.Generator().manual_seed(R + K), dtype=torch.int32)
    img = F8.encode_image(exps, layout, R, K)
    back, pad = F8.read_image(img, layout, R, K)
    assert torch.equal(back, exps) and int(pad.count_nonzero()) == 0
    if layout == 2:
        assert torch.equal(img.reshape(R, K // 32).to(torch.int32) - 127, exps) and pad.numel() == 0
        return
    assert torch.equal(img, F8.header_image(exps, layout, R, K))
    assert pad.numel() == img.numel() - R * (K // 32) and (pad.numel() > 0) == (R % 256 != 0)
    img[:] = 255                                                          # read_image returns exactly the complement
    assert int(F8.read_image(img, layout, R, K)[1].numel()) == pad.numel()


@pytest.mark.parametrize("M,N,K", [(300, 264, 384), (257, 1000, 128), (2040, 2056, 256)])
def test_bf16_zero_bar_families_are_exact(M, N, K):
    for fam in F8.ZERO_BAR:
        for wide in ((True, False) if fam == "selector" else (True,)):
            d = F8.zero_family(fam, M, N, K, wide)
            assert F8.zero_exact(d), fam
            acc = F8.zero_product(d)
            ref = F8.gemm_f8(d["Aq"], d["Ae"], d["Bq"], d["Be"])
            assert torch.equal(acc.double(), ref.out)                    # the cheap fp32 product IS the float64 one
            forms = [acc] if fam == "selector" and wide else [acc, acc + d["bias"][None, :], acc + d["R"], acc + d["bias"][None, :] + d["R"]]
            for want in forms:
                assert torch.equal(want, want.bfloat16().float()), (fam, wide)
            assert float(acc.abs().max()) > 8 and int((acc != 0).sum()) > acc.numel() // 3          # not vacuous
    d = F8.zero_family("selector", M, N, K, True)
    a = F8.decode(d["Aq"], d["Ae"])
    assert bool(((a != 0).sum(1) == 1).all()) and torch.equal(a.abs().argmax(1), (5 * torch.arange(M) + 3) % K)
    assert len(set(d["Ae"].reshape(-1).tolist())) == 6 and len(set(d["Be"].reshape(-1).tolist())) == 6


@pytest.mark.parametrize("M,N,K", [(300, 256, 256), (2040, 2048, 384)])
def test_intsum_is_exact_in_fp32_and_holds_the_engineered_blocks(M, N, K):
    d = F8.zero_family("intsum", M, N, K)
    assert F8.zero_exact(d, unit=1.0)
    z = F8.zero_product(d)
    assert torch.equal(z.double(), F8.gemm_f8(d["Aq"], d["Ae"], d["Bq"], d["Be"]).out)
    assert not torch.equal(z, z.bfloat16().float())                      # exact in fp32, NOT in bf16: a bf16 round trip before the quantiser shows
    codes, e = MX.quantize(z)
    m = torch.arange(M)
    blk = z.abs().reshape(M, N // 32, 32).amax(-1)
    assert bool((blk[m % 64 == 7] == 4.0).all()) and bool((e[m % 64 == 7] == 2 - 8).all())          # the maximum is 2^2 exactly
    sat = m % 64 == 11
    assert bool((blk[sat] == 15.0).all()) and bool((e[sat] == 3 - 8).all())
    hit = z[sat].abs() == 15.0
    assert bool(hit.any()) and bool(((codes[sat][hit] & 0x7F) == 0x7E).all())                      # 480 after scaling: saturated to 448
    # the rules accept the rule's own output at bar 0 and name nothing movable
    assert F8.quant_errors(codes, e, z.double(), 0.0)[:2] == (0, 0)
    blk_m, el_m = F8.can_move(z.double(), 0.0)
    assert not bool(blk_m.any()) and not bool(el_m.any())
    assert torch.equal(F8.codes_at(z.double(), e), codes)


def test_quantised_output_rules_reject_what_they_should():
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(64, 256, generator=g, dtype=F64) * torch.logspace(-3, 3, 64, dtype=F64)[:, None]
    ref[0, :32] = 0.0
    ref[1, 32:64] *= 1e-4                                                 # scaled values deep in the subnormal range next to ...
    ref[1, 40] = 300.0
    bar = 4.0 * Bar.U32 * ref.abs() + 1e-30
    codes, e = MX.quantize(ref.float())
    assert F8.quant_errors(codes, e, ref, bar)[:2] == (0, 0)
    assert F8.quant_errors(codes, e + 1, ref, bar)[0] > 60 * 8            # a wrong exponent everywhere (the all-zero block's -127 may move)
    bumped = codes.clone()
    bumped[5, 7] += 1                                                     # one code one step off
    assert F8.quant_errors(bumped, e, ref, bar)[1] == 1
    trunc = F8.codes_at(ref * (1 - 2.0 ** -5), e)                         # a systematic pull towards zero, well inside one step
    assert F8.quant_errors(trunc, e, ref, bar)[1] > 1000
    # the clamp: a block maximum in (448, 512) 2^e saturates, and only there does the bound open
    r2 = torch.full((1, 32), 1.0, dtype=F64)
    r2[0, 0] = 500.0
    c2, e2 = MX.quantize(r2.float())
    assert int(e2[0, 0]) == 0 and int(c2[0, 0]) == 0x7E and F8.quant_errors(c2, e2, r2, 1e-9)[:2] == (0, 0)
    c2[0, 0] = 0x76                                                       # 224: not what a clamp gives
    assert F8.quant_errors(c2, e2, r2, 1e-9)[1] == 1
    lo, hi = F8.admissible_exps(torch.tensor([[4.0] * 32, [4.5] * 32], dtype=F64), 1e-6)
    assert lo.tolist() == [[-7], [-6]] and hi.tolist() == [[-6], [-6]]    # a maximum on a power of two may land on either side; one off it may not


def test_e4m3_step():
    s = torch.tensor([0.0, 2.0 ** -10, 2.0 ** -6, 0.99, 1.0, 1.99, 255.0, 256.0, 448.0, 500.0], dtype=F64)
    assert F8.e4m3_step(s).tolist() == [2.0 ** -9, 2.0 ** -9, 2.0 ** -9, 2.0 ** -4, 2.0 ** -3, 2.0 ** -3, 16.0, 32.0, 32.0, 32.0]
    t = F8.E4M3[:127]                                                     # the positive codes in order: the step is the gap to the next one
    assert torch.equal(F8.e4m3_step(t[:-1]), t[1:] - t[:-1])


def test_constructed_blocks_sit_where_they_claim():
    for dt in (F32, BF16):
        x = F8.constructed_blocks(dt)
        codes, e = MX.quantize(x.float())
        v = codes.view(torch.float8_e4m3fn).float()
        assert e[:6, 0].tolist() == [k - 8 for k in (-20, -1, 0, 1, 7, 30)] and bool((v[:6, 0] == 256.0).all())
        assert bool((v[6:12:2, 0] == 448.0).all()) and bool((v[7:12:2, 0] == -448.0).all()) and bool((v[7:12:2, 1] == 448.0).all())
        assert bool((v[12:15, 0] == 448.0).all()) and bool((v[12:15, 1] == -448.0).all())          # 510 after scaling: clamped
        ties = x[15].double()[1:]
        assert bool((F8.E4M3[codes[15, 1:].long()] != ties).all())       # none is representable: each was rounded, to the even neighbour
        assert bool(((codes[15, 1:] & 1) == 0).all())
        assert int(e[-1, 0]) == -127 and int(codes[-1].count_nonzero()) > 4                          # subnormal inputs: e = -127, codes not all zero
        assert codes[17].tolist()[:4] == [0x78, 0x80, 0x00, 0x80] and bool((codes[18] == 0x80).all())                 # -0.0 keeps its sign


def _norm_case(rms, d, rows, fam):
    from test_bytemovers_gpu import family, gen
    x = family(fam, rows, d, BF16, 13, dev="cpu")
    w = (1 + 0.1 * torch.randn(d, generator=gen(14 + d))).to(BF16)
    b = None if rms else (0.1 * torch.randn(d, generator=gen(15 + d))).to(BF16)
    return x, w, b


@pytest.mark.parametrize("d", F8.NORM_D)
@pytest.mark.parametrize("rms", (False, True), ids=("layernorm", "rmsnorm"))
def test_norm_bar_leaves_almost_every_code_determined(rms, d):
    """The set the GPU test exempts from equality is computed from the reference and the bar alone and stays under the family's MOVE_CAP of the
    elements and of the blocks (or one of either, where a case is small) in every case.  const under LayerNorm exempts nothing: its premise, that the
    float64 result is the bias itself, is checked instead."""
    for rows, fam, _, _ in F8.norm_cases(rms, d):
        x, w, b = _norm_case(rms, d, rows, fam)
        ref, c32, _, _ = F8.norm_ref(x, w, b, rms)
        if F8.norm_exact(rms, fam):
            assert torch.equal(ref, b.double().expand_as(ref)) and torch.equal(c32, b.float().expand_as(c32))
            continue
        blk, el = F8.can_move(ref, Bar.fp32_bar(ref, c32))
        cap_el, cap_blk = F8.MOVE_CAP[fam]
        sb, se = float(blk.double().mean()), float(el.double().mean())
        print(f"{fam} rows {rows}: {sb:.2e} of the blocks, {se:.2e} of the elements can move")
        assert int(blk.sum()) <= max(1, cap_blk * blk.numel()) and int(el.sum()) <= max(1, cap_el * el.numel()), (rows, fam, sb, se)


def test_norm_bar_share_on_plain_rows():
    """LayerNorm of 3 randn + 0.5 rows (tests/test_fp8_gpu.py's input) at d = 768 and 4096: under randn's MOVE_CAP of the elements (4e-4 measured), next to none of the blocks."""
    for d in (768, 4096):
        g = torch.Generator().manual_seed(d)
        x = (torch.randn(300, d, generator=g) * 3 + 0.5).to(BF16)
        w, b = (1 + 0.1 * torch.randn(d, generator=g)).to(BF16), torch.randn(d, generator=g).to(BF16)
        ref, c32, _, _ = F8.norm_ref(x, w, b, False)
        blk, el = F8.can_move(ref, Bar.fp32_bar(ref, c32))
        assert float(el.double().mean()) < F8.MOVE_CAP["randn"][0] and float(blk.double().mean()) < 1e-4


def test_library_exports_the_plan_predicate():
    from avllm import lib as L
    assert "avllm_gemm_f8_takes_fast" in L.EXPORTS and "avllm_gemm_f8_takes_quantised_output" in L.EXPORTS


def _one_step(a_vals, b_vals):
    """One 128-wide row pair from the leading values (the rest zero), all scales 0."""
    a, b = torch.zeros(1, 128), torch.zeros(1, 128)
    a[0, :len(a_vals)] = torch.tensor(a_vals)
    b[0, :len(b_vals)] = torch.tensor(b_vals)
    z = torch.zeros(1, 4, dtype=torch.int32)
    return F8.code_of(a), z, F8.code_of(b), z


def test_mfma_group_loss_restates_the_measured_cut():
    """The cases of profiles/r16_fp8_mfma_probe.txt: what the device dropped is within the bound, and the bound is 0 where it dropped nothing."""
    loss = lambda a, b: float(F8.mfma_group_loss(*_one_step(a, b)))
    # beside P = 2^16: 2^3 survives (exponent sum 3 is 13 below: cut at 2^3, a multiple of it), 2^2 is lost whole, 1.875 2^5 loses 4 of its 60
    assert loss([256.0, 256.0, 1.0], [256.0, -256.0, 8.0]) == 0.0
    assert loss([256.0, 256.0, 1.0], [256.0, -256.0, 4.0]) == 4.0
    assert loss([256.0, 256.0, 32.0], [256.0, -256.0, 1.875]) == 4.0
    assert loss([256.0, 256.0, 2.0 ** -6], [256.0, -256.0, 2.0 ** -6]) == 2.0 ** -12                 # at most the product itself
    # within 7 exponents of the largest: 8 significant bits fit above the cut
    assert loss([256.0, 256.0, 2.0], [256.0, -256.0, 1.875 * 128]) == 0.0
    # the small product in ANOTHER group of 8 is untouched, whichever block it sits in
    a, b = [256.0, 256.0] + [0.0] * 6 + [1.0], [256.0, -256.0] + [0.0] * 6 + [1.0]
    assert loss(a, b) == 0.0
    # a zero operand sets no exponent; a subnormal one counts as 2^-6
    assert loss([0.0, 1.0], [448.0, 2.0 ** -9]) == 0.0
    assert loss([2.0 ** -9, 2.0 ** -9, 2.0 ** -6], [256.0, -256.0, 2.0 ** -6]) == 2.0 ** -12         # cut at 2^(2 - 13), although P is only 2^-1
    assert loss([2.0 ** -6, 2.0 ** -6, 2.0 ** -6], [32.0, -32.0, 2.0 ** -6]) == 0.0                  # the same P from normal operands: cut at 2^-14
    # block scales move a group as a whole
    Aq, z, Bq, _ = _one_step([256.0, 256.0, 1.0], [256.0, -256.0, 4.0])
    assert float(F8.mfma_group_loss(Aq, z + 3, Bq, z - 1)) == 4.0 * 4.0
    for fam in F8.ZERO_BAR + ("intsum",):
        d = F8.zero_family(fam, 65, 72, 256)
        assert float(F8.mfma_group_loss(d["Aq"], d["Ae"], d["Bq"], d["Be"]).max()) == 0.0            # the zero-bar families stay zero-bar


def test_ln_rstd_bar_covers_the_host_fp32_evaluation():
    g = torch.Generator().manual_seed(1)
    for d, off in ((128, 0.0), (4096, 8.0), (8192, 8.0)):
        x = (torch.randn(65, d, generator=g) + off).to(BF16)
        _, _, r64, r32 = F8.norm_ref(x, torch.ones(d), torch.zeros(d), False)
        rel = ((r32.double() - r64) / r64).abs()
        assert bool((rel <= Bar.ln_rstd_bar(x.double())).all()) and float(Bar.ln_rstd_bar(x.double()).max()) < 2e-3
