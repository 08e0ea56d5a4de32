"""The yardsticks of tests/test_select_pin_gpu.py, checked on the host alone: every host emulation of a token-selection kernel's documented
float32 arithmetic (refs64_select) stays under its derived bar (bars.py, "token selection against float64") on every family, every planted
fault exceeds the bar or fails the check, and the caps on undecided draws hold on the float64 reference itself."""
import numpy as np
import pytest
import torch

import bars
import refs64_select as R
from sample_ref import rows as randn3

VS = [1000, 4097, 151936]
CFGS = R.SAMPLE_CFGS
STEPS = range(64)
SEED = 1234


def finite(a):
    return torch.isfinite(torch.as_tensor(a))


# ---------------------------------------------------------------- log-probabilities and entropies
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_online_state_emulation_is_under_the_bars_and_faults_are_not(fam, V):
    x = R.family(fam, V, seed=V)
    t = 0.7
    y32 = (x[0] / torch.tensor(t)).numpy()
    order = np.argsort(-y32, kind="stable")
    tok = int(order[min(2, V - 1)])
    tk = torch.tensor([tok])
    lp64, ent64 = R.row_scores64(x, tk, t)
    lp32, ent32 = R.row_scores64(x, tk, t, dtype=torch.float32)
    y64 = torch.as_tensor(y32).double()[None]
    fin = y64[0][torch.isfinite(y64[0])]
    bar_lp = bars.select_logprob_bar(lp64, lp32, V, sizes=(fin, fin - fin.max(), lp64))
    bar_ent = bars.select_entropy_bar(y64, ent64, ent32)
    lp, ent = R.mst_scores(*R.mst_emul(y32), y32[tok])
    r_lp, r_ent = abs(lp - float(lp64)) / bar_lp, abs(ent - float(ent64)) / bar_ent
    print(f"RATIO row_scores emulation {fam} V={V}: logprob {r_lp:.3f} entropy {r_ent:.3f} (bars {bar_lp:.2e} {bar_ent:.2e})")
    assert r_lp <= 1.0 and r_ent <= 1.0
    if fam in ("randn", "banned"):
        # one element (the tenth largest) left out of the sums; a skipped raise in the merge
        lp_f, ent_f = R.mst_scores(*R.mst_emul(y32, leave_out=int(order[9])), y32[tok])
        assert abs(lp_f - float(lp64)) > bar_lp or abs(ent_f - float(ent64)) > bar_ent
        lp_f, ent_f = R.mst_scores(*R.mst_emul(y32, skip_raise=True), y32[tok])
        assert abs(lp_f - float(lp64)) > bar_lp and abs(ent_f - float(ent64)) > bar_ent


@pytest.mark.parametrize("V", [97, 4097, 151936])
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_log_softmax_and_beam_score_emulations(fam, V):
    x = R.family(fam, V, seed=V + 1, rows=2)
    bs = torch.tensor([-1.25, -7.5])
    ref = R.log_softmax64(x)
    ok = finite(ref)
    cpu = torch.log_softmax(x, -1)
    mx = x.double().max(-1, keepdim=True).values
    d = (x.double() - mx)[ok]
    bar = bars.select_logprob_bar(ref[ok], cpu[ok], V, sizes=(d, ref[ok]))
    got = R.log_softmax32(x)
    assert torch.equal(torch.isinf(got), ~ok)
    r = float((got.double() - ref)[ok].abs().max()) / bar
    s64 = R.beam_scores64(x, bs)
    bar_b = bars.select_logprob_bar(s64[ok], (cpu + bs[:, None])[ok], V, sizes=(d, ref[ok], s64[ok]))
    e = lambda s: float((s.double() - s64)[ok].abs().max())  # noqa: E731
    rb = e(R.beam_scores32(x, bs)) / bar_b
    print(f"RATIO log_softmax emulation {fam} V={V}: {r:.3f}; beam score emulation {rb:.3f} (bars {bar:.2e} {bar_b:.2e})")
    assert r <= 1.0 and rb <= 1.0
    if V > R.SEG and fam in ("randn", "banned"):
        heavy = int((R.log_softmax64(x[:1]).exp().view(-1)[: V // R.SEG * R.SEG].view(-1, R.SEG).sum(1)).argmax())
        assert e(R.beam_scores32(x, bs, drop_seg=heavy)) > bar_b                      # a dropped segment
    if V > R.SEG and fam in ("randn", "pm80"):
        assert e(R.beam_scores32(x, bs, rescale=False)) > bar_b                        # a segment's sum not rescaled to the row maximum


# ---------------------------------------------------------------- beam_topk validity
def test_beam_validity_rule_catches_planted_faults():
    V, nb, k = 8193, 3, 6
    x = R.family("randn", V, seed=5, rows=nb)
    bs = torch.tensor([-0.5, -1.0, -0.25])
    s64 = R.beam_scores64(x, bs).view(-1)
    cpu = (torch.log_softmax(x, -1) + bs[:, None]).view(-1)
    bar = bars.select_logprob_bar(s64, cpu, V, sizes=(s64,))
    s32 = R.beam_scores32(x, bs).view(-1)
    order = R.beam_order(s32, k + 1)
    good, nxt = order[:k], order[k]
    ok, why = R.beam_valid(s32[good], good, s64, k, bar)
    assert ok, why
    swapped = good.copy()
    swapped[0] = nxt                                                                   # one candidate replaced by the (k+1)-th
    resort = swapped[np.argsort(-s32[swapped].numpy(), kind="stable")]
    assert not R.beam_valid(s32[resort], resort, s64, k, bar)[0]
    assert not R.beam_valid(s32[good[[0, 0, 2, 3, 4, 5]]], good[[0, 0, 2, 3, 4, 5]], s64, k, bar)[0]      # a pair twice
    assert not R.beam_valid(s32[good] + 1e-3, good, s64, k, bar)[0]                    # scores off
    assert not R.beam_valid(s32[good[::-1].copy()], good[::-1].copy(), s64, k, bar)[0]               # ascending
    nan_one = s32[good].clone()
    nan_one[2] = float("nan")                                                          # a NaN score, as a read past V into the NaN padding gives
    assert R.beam_valid(nan_one, good, s64, k, bar) == (False, "NaN scores")
    assert R.beam_valid(torch.full((k,), float("nan")), good, s64, k, bar) == (False, "NaN scores")
    assert not R.beam_valid(s32[good], good, s64, k, float("nan"))[0]                  # and a NaN bar passes nothing
    # the exact family: the bar is 0 and ties must come in flat-index order
    lp = R.exact_logprobs(nb, V, seed=6)
    lp[0, [4095, 4096]] = lp[1, 1023] = lp[1, 1024] = -0.5
    sx = R.beam_scores64(lp, torch.zeros(nb), logprobs=True).view(-1)
    want = R.beam_order(sx, 4)
    assert want.tolist() == [4095, 4096, V + 1023, V + 1024]
    assert R.beam_valid(sx[want].float(), want, sx, 4, 0.0)[0]
    wrong = want[[1, 0, 2, 3]]                                                         # ties returned in the wrong index order
    assert not R.beam_valid(sx[wrong].float(), wrong, sx, 4, 0.0)[0]
    # every sum of the exact family is exact in float32
    b = R.exact_beam_scores(nb, seed=7)
    assert torch.equal((lp + b[:, None]).double(), R.beam_scores64(lp, b, logprobs=True))


# ---------------------------------------------------------------- the draw
def emulated_tokens(row, t, k, p, steps, rs, k_off=0, p_short=False, **fault):
    y32 = (np.asarray(row, np.float32) / np.float32(t)).astype(np.float32)
    keep, _ = R.kept(row, t, k + k_off if 0 < k < len(row) else k, 1.0)               # a top-k threshold one rank off
    if p < 1.0:
        keep = R.emul_top_p_keep(y32, keep, p)
        if p_short:                                                                    # a top-p prefix one token short
            keep = keep & (y32 > y32[keep].min())
    w = R.masses32(y32, keep)
    return [R.emul_draw(y32, keep, R.u24(SEED, rs, st), w=w, **fault) for st in steps]


@pytest.mark.parametrize("V", [1000, 36784, 36800, 151936])
def test_draw_emulation_stays_in_its_brackets_and_faults_do_not(V):
    x = randn3(2, V, seed=V).numpy()
    worst = 0.0
    for t, k, p in ((0.7, 50, 0.9), (1.0, 0, 0.95), (1.0, 0, 1.0), (1.3, 2049, 0.95), (1.0, 50, 1.0)):
        for b in range(2):
            c = R.check_draws(x[b], t, k, p, SEED, b, STEPS, emulated_tokens(x[b], t, k, p, STEPS, b))
            assert not c["errors"], (V, t, k, p, b, c["errors"][:3])
            worst = max(worst, c["ratio"])
            for fault in (dict(shift=1), dict(tile_shift=1), dict(inclusive_bug=True)):
                if V <= R.TILE * 4 and "tile_shift" in fault and k:
                    continue
                bad = R.check_draws(x[b], t, k, p, SEED, b, STEPS, emulated_tokens(x[b], t, k, p, STEPS, b, **fault))
                assert bad["errors"], (V, t, k, p, b, fault)
        # a wrong kept set moves the CDF by the mass of one boundary token: it shows on the draws that land near it, so over 256 steps and both rows
        faults = ([dict(k_off=-1)] if 0 < k < V and p >= 1.0 else []) + ([dict(p_short=True)] if p < 1.0 else [])   # (under top-p the k-th token
        for fault in faults:                                                                                         # is not kept: no draw shows it)
            more = range(256)
            caught = sum(len(R.check_draws(x[b], t, k, p, SEED, b, more, emulated_tokens(x[b], t, k, p, more, b, **fault))["errors"]) for b in range(2))
            assert caught, (V, t, k, p, fault)
    print(f"RATIO draw emulation V={V}: worst distance outside an interval / tol {worst:.3f}")


@pytest.mark.parametrize("V", R.SAMPLE_VS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_undecided_caps_hold_on_the_reference_alone(V, dtype):
    """The caps of the GPU pin on the float64 draws themselves, over the very rows, seeds and steps the pin uses (whether a draw is decided does not
    depend on the token a kernel returns, so this is the pin's cap assertion, made where it can be read without a GPU)."""
    x = R.sample_input(V, dtype).float().numpy()
    steps, n = range(R.SAMPLE_STEPS), 4 * R.SAMPLE_STEPS
    for t, k, p in R.SAMPLE_CFGS:
        und = plain = 0
        for b, rs in enumerate(R.SAMPLE_ROW_SEEDS):
            c = R.check_draws(x[b], t, k, p, R.SAMPLE_SEED, rs, steps, R.draws64(x[b], t, k, p, R.SAMPLE_SEED, rs, steps))
            assert not c["errors"], c["errors"][:3]
            und, plain = und + c["undecided"], plain + c["undecided_same_sets"]
        print(f"UNDECIDED reference V={V} {dtype} {(t, k, p)}: {und} of {n} (by the equal-sets rule alone: {plain})")
        assert und <= R.undecided_cap(V, k, n), (V, t, k, p, und)


def test_sample_logprob_emulation():
    for V in (1000, 151936):
        x = randn3(2, V, seed=V + 1).numpy()
        for t, k, p in CFGS:
            for b in range(2):
                keep, _ = R.kept(x[b], t, k, p)
                y32 = (x[b] / np.float32(t)).astype(np.float32)
                tok = int(np.nonzero(keep)[0][-1])
                ref = R.sample_logprob64(y32.astype(np.float64), keep, tok)
                z = torch.as_tensor(y32[keep])
                cpu = float(torch.log_softmax(z, 0)[-1])
                bar = bars.select_logprob_bar(torch.tensor([ref]), torch.tensor([cpu]), int(keep.sum()), sizes=(z.double(), z.double() - z.double().max(), ref))
                assert abs(R.sample_logprob32(y32, keep, tok) - ref) <= bar


def test_top_k_1_reference_reads_nan_as_minus_inf():
    import refs64
    x = np.array([np.nan, 1.0, 3.0, np.nan, 3.0], np.float32)
    keep, prob = R.kept(x, 0.5, 1, 0.9)
    assert np.nonzero(keep)[0].tolist() == [2] == refs64.argmax_rows(torch.tensor(x)[None]).tolist()
    keep, prob = R.kept(x, 1.0, 0, 1.0)
    assert not keep[0] and not keep[3] and prob[0] == 0.0


def test_ratio_helpers_reject_nan():
    """A NaN result compares False with every bound and max(0.0, nan) is 0.0: the helpers every pin ratio goes through must fail on it."""
    nan, inf = float("nan"), float("inf")
    assert R.ratio(torch.tensor([1e-6, -2e-6]), 1e-5) == pytest.approx(0.2) and R.ratio(torch.zeros(0), 1e-5) == 0.0
    assert R.ratio(0.0, 0.0) == 0.0 and R.ratio(1e-9, 0.0) == inf
    for bad in (nan, inf, torch.tensor([0.0, nan]), torch.tensor([-inf, 0.0])):
        with pytest.raises(AssertionError):
            R.ratio(bad, 1e-5)
    with pytest.raises(AssertionError):
        R.ratio(0.0, nan)
    assert R.worst_of(0.5, 0.25) == 0.5 and R.worst_of(0.5, inf) == inf
    with pytest.raises(AssertionError):
        R.worst_of(0.5, nan)
    # the sample_rows log-probability: a NaN or infinite score fails, a token outside both kept sets gives inf, a good one a ratio below 1
    x = randn3(1, 1000, seed=3).numpy()[0]
    t, k, p = 0.7, 50, 0.9
    keep, _ = R.kept(x, t, k, p)
    y32 = (x / np.float32(t)).astype(np.float32)
    toks = np.nonzero(keep)[0][:4]
    lps = np.array([R.sample_logprob32(y32, keep, int(tk)) for tk in toks], np.float32)
    assert R.sample_logprob_ratio(x, t, k, p, toks, lps) <= 1.0
    assert R.sample_logprob_ratio(x, t, k, p, toks, lps + np.float32(1e-3)) > 1.0
    assert R.sample_logprob_ratio(x, t, k, p, np.array([int(np.nonzero(~keep)[0][0])]), lps[:1]) == inf
    for bad in (nan, -inf):
        broken = lps.copy()
        broken[1] = bad
        with pytest.raises(AssertionError):
            R.sample_logprob_ratio(x, t, k, p, toks, broken)
