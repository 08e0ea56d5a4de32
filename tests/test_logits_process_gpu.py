"""ops.logits_process (csrc/logits_process.hip) against test_logits_process_cpu.restate, the CPU restatement of HF's
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor in the gather / compute / scatter form
(itself held to HF's classes there), bit for bit; the log-softmax mode beam search uses; and ops.beam_topk(logprobs=True)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars  # noqa: E402
from avllm import ops  # noqa: E402
from test_logits_process_cpu import ALPHABET, EOS, NEG_INF, NGRAMS, PENALTIES, VOCABS, lengths, make, restate, same_bits  # noqa: E402


def run(scores, hist, cur, p, n, m, eos, **kw):
    """The kernel on a device copy; the history tensor is wider than cur, so entries past cur must not be read."""
    rows = scores.shape[0]
    wide = torch.full((rows, max(cur + 5, 8)), int(ALPHABET[0]), dtype=torch.int64)
    wide[:, :cur] = hist
    return ops.logits_process(scores.cuda(), wide.cuda(), cur, p, n, m, eos=eos, **kw).cpu()


@pytest.mark.parametrize("p", PENALTIES)
@pytest.mark.parametrize("V", VOCABS)
def test_matches_restatement_bit_for_bit(dev, V, p):
    checked = 0
    for n in NGRAMS:
        for cur in lengths(n):
            for m in (cur, cur + 1):                   # min_new_tokens off (cur >= m) and on (cur < m)
                scores, hist = make(V, cur, seed=V + 31 * n + cur)
                want = restate(scores, hist, p, n, m, EOS)
                got = run(scores, hist, cur, p, n, m, EOS)
                assert same_bits(got, want), (V, p, n, cur, m, (got != want).nonzero()[:5])
                assert torch.equal(torch.isinf(got), torch.isinf(want))
                again = run(scores, hist, cur, p, n, m, EOS)
                assert same_bits(again, got), "two launches must give identical bits"
                checked += 1
    assert checked == sum(2 * len(lengths(n)) for n in NGRAMS)


def test_repeated_token_is_penalised_once(dev):
    """The double-penalty case: one token 64 times in the history, p = 1.3: its score is divided (or multiplied) by 1.3 once, not 64 times."""
    V, tok = 32000, 42
    for sign in (1.0, -1.0):
        scores = torch.randn(2, V, generator=torch.Generator().manual_seed(5)) * 4
        scores[:, tok] = sign * 2.5
        hist = torch.full((2, 64), tok, dtype=torch.int64)
        got = run(scores, hist, 64, 1.3, 0, 0, None)
        want = scores.clone()
        want[:, tok] = scores[:, tok] / 1.3 if sign > 0 else scores[:, tok] * 1.3
        assert same_bits(got, want), (sign, got[:, tok], want[:, tok])
        assert same_bits(got, restate(scores, hist, 1.3, 0, 0, None))


def test_no_eos_id_and_each_processor_alone(dev):
    scores, hist = make(32000, 300, seed=9)
    for p, n, m, eos in ((1.3, 0, 0, EOS), (1.0, 2, 0, EOS), (1.0, 0, 400, EOS), (1.0, 0, 400, None), (1.3, 4, 400, None)):
        got = run(scores, hist, 300, p, n, m, eos)
        assert same_bits(got, restate(scores, hist, p, n, m, eos)), (p, n, m, eos)
    assert same_bits(run(scores, hist, 300, 1.0, 0, 400, None), scores)


def test_append_stores_the_last_token_first(dev):
    """append: the token for position cur-1 comes from a [rows] tensor and is written into the history by the launch itself."""
    scores, hist = make(32000, 40, seed=13, rows=4)
    d_hist = torch.zeros(4, 64, dtype=torch.int64)
    d_hist[:, :39] = hist[:, :39]
    d_hist = d_hist.cuda()
    got = ops.logits_process(scores.cuda(), d_hist, 40, 1.3, 2, 0, eos=EOS, append=hist[:, 39].contiguous().cuda()).cpu()
    assert torch.equal(d_hist.cpu()[:, :40], hist) and (d_hist.cpu()[:, 40:] == 0).all()
    assert same_bits(got, restate(scores, hist, 1.3, 2, 0, EOS))


def test_history_length_in_device_memory(dev):
    scores, hist = make(32000, 300, seed=17)
    cur = torch.tensor([300], dtype=torch.int32, device="cuda")
    wide = torch.zeros(3, 512, dtype=torch.int64)
    wide[:, :300] = hist
    got = ops.logits_process(scores.cuda(), wide.cuda(), cur, 1.3, 4, 301, eos=EOS).cpu()
    assert same_bits(got, restate(scores, hist, 1.3, 4, 301, EOS))


def test_strided_rows_and_bf16(dev):
    scores, hist = make(32000, 300, seed=21)
    big = torch.zeros(3, 32000 + 77)
    big[:, 5:5 + 32000] = scores
    d = big.cuda()
    ops.logits_process(d[:, 5:5 + 32000], hist.cuda(), 300, 1.3, 2, 0, eos=EOS)
    out = d.cpu()
    assert same_bits(out[:, 5:5 + 32000], restate(scores, hist, 1.3, 2, 0, EOS))
    assert (out[:, :5] == 0).all() and (out[:, 5 + 32000:] == 0).all()
    # bf16 scores: the arithmetic is fp32 on the widened value with the fp32 penalty, rounded once to bf16
    sb = scores.bfloat16()
    f = sb.float()
    g = torch.gather(f, 1, hist)
    want = f.scatter(1, hist, torch.where(g < 0, g * 1.3, g / 1.3)).bfloat16()
    want = restate(want, hist, 1.0, 2, 301, EOS)
    got = ops.logits_process(sb.cuda(), hist.cuda(), 300, 1.3, 2, 301, eos=EOS).cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("V", VOCABS)
def test_log_softmax_mode(dev, V):
    """Beam search's order: the row becomes its log-softmax (normaliser of the unprocessed logits), then the processors run on the
    log-probabilities.  Untouched entries agree with torch.log_softmax within the bar tests/test_beam_gpu.py uses for the same arithmetic
    (the kernel and torch sum in different orders); touched entries are the processors applied to the kernel's own value, exactly."""
    for n in (0, 2, 4):
        for cur in (0, 1, 300, 1024):
            scores, hist = make(V, cur, seed=3 * V + cur + n)
            ref = torch.log_softmax(scores.double(), dim=-1)
            own = run(scores, hist, cur, 1.0, 0, 0, None, log_softmax=True)
            # float64 under the derived bar of tests/bars.py where that is not larger than the earlier hand-set 8 eps (max + 1) + 1e-6, else that
            d = scores.double() - scores.double().max(-1, keepdim=True).values
            tol = min(8 * torch.finfo(torch.float32).eps * (ref.abs().max().item() + 1.0) + 1e-6,
                      bars.select_logprob_bar(ref, torch.log_softmax(scores, dim=-1), V, sizes=(d, ref)))
            assert (own.double() - ref).abs().max().item() <= tol, (V, cur, (own.double() - ref).abs().max().item(), tol)
            for p in PENALTIES:
                m = cur + 1 if n else cur
                got = run(scores, hist, cur, p, n, m, EOS, log_softmax=True)
                assert same_bits(got, restate(own, hist, p, n, m, EOS)), (V, n, cur, p)
                assert same_bits(got, run(scores, hist, cur, p, n, m, EOS, log_softmax=True))
                if cur:                                # every log-probability is negative: the penalty multiplies
                    t = int(hist[0, 0])
                    assert got[0, t] == NEG_INF or got[0, t] == own[0, t] * torch.tensor(p, dtype=torch.float32)


def test_beam_topk_on_log_probabilities(dev):
    """beam_topk(logprobs=True) adds the beam score to the row as it is; a banned (-inf) entry is returned only when an item has fewer
    than k finite candidates."""
    g = torch.Generator().manual_seed(2)
    for V, nb, B in ((97, 2, 3), (32000, 4, 2), (128256, 4, 2)):
        k = 2 * nb
        lp = torch.log_softmax(torch.randn(B * nb, V, generator=g) * 4, dim=-1)
        lp[:, ALPHABET] = NEG_INF
        top = torch.topk(lp, 3, dim=1)[1]
        lp[torch.arange(B * nb)[:, None], top[:, :2]] = NEG_INF      # the two best of every row are banned
        sc = -torch.rand(B * nb, generator=g) * 3
        want_s, want_i = torch.topk((lp + sc[:, None]).view(B, nb * V), k, dim=1)
        s, b, t = (x.cpu() for x in ops.beam_topk(lp.cuda(), sc.cuda(), nb, k, logprobs=True))
        assert same_bits(s, want_s)
        assert torch.isfinite(s).all()
        distinct = torch.ones_like(want_s, dtype=torch.bool)
        distinct[:, 1:] &= want_s[:, 1:] != want_s[:, :-1]
        distinct[:, :-1] &= want_s[:, :-1] != want_s[:, 1:]
        assert torch.equal((b.long() * V + t)[distinct], want_i[distinct])
    # one beam, three finite entries, k = 4: the finite ones first, in order, then a banned one
    lp = torch.full((1, 97), NEG_INF)
    lp[0, [5, 50, 90]] = torch.tensor([-2.0, -0.5, -1.0])
    s, b, t = (x.cpu() for x in ops.beam_topk(lp.cuda(), torch.zeros(1).cuda(), 1, 4, logprobs=True))
    assert t[0, :3].tolist() == [50, 90, 5] and s[0, :3].tolist() == [-0.5, -1.0, -2.0] and s[0, 3] == NEG_INF


def test_history_longer_than_the_limit_is_an_error(dev):
    assert ops.LOGITS_PROCESS_MAX_HISTORY >= 1024
    n = ops.LOGITS_PROCESS_MAX_HISTORY + 1
    scores = torch.zeros(2, 97, device="cuda")
    hist = torch.zeros(2, n, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="at most"):
        ops.logits_process(scores, hist, n, 1.3, 2, 0, eos=EOS)
    with pytest.raises(ValueError, match="at most"):       # a length in device memory: the row stride bounds it
        ops.logits_process(scores, hist, torch.zeros(1, dtype=torch.int32, device="cuda"), 1.3, 2, 0, eos=EOS)
    with pytest.raises(ValueError):
        ops.logits_process(scores, hist[:, :8], 9, 1.3, 2, 0, eos=EOS)
    assert (scores == 0).all()
