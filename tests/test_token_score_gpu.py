"""ops.row_scores (csrc/token_score.hip): the chosen token's log-probability and the row's entropy in one pass, against float64 on the same
float32 values (the division by the float32 temperature included), at every vector edge (V below, at and above one vector per lane; row
strides that break the 16-byte alignment), with banned (-inf) entries, and the log-probability-input mode beam search uses.

Bar: per row the derived bars of tests/bars.py (select_logprob_bar, select_entropy_bar), capped at the earlier hand-set 1e-4 absolute, which
stays the bar of the log-probability-input mode and of tokens=None."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from avllm import lib as L  # noqa: E402
import bars  # noqa: E402
from avllm import ops  # noqa: E402
from refs64_select import row_scores64 as reference  # noqa: E402  (float64 on the float32 values: (logprob, entropy) per row)

TOL = 1e-4
VS = [1, 63, 64, 65, 1000, 4097, 32000, 128256, 151936]
NEG = float("-inf")
WORST = {"logprob": 0.0, "entropy": 0.0}


def pattern_rows(V, seed):
    """The input families as rows [P, V] with one chosen token each."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.randn(V, generator=g) * 4  # noqa: E731
    pick = lambda: int(torch.randint(0, V, (1,), generator=g))  # noqa: E731
    rows, toks = [], []

    def add(r, t):
        rows.append(r); toks.append(t)
    add(rnd(), pick())                                                  # plain
    r, j = rnd(), pick()
    r[j] = r.max() + 60.0
    add(r, j)                                                           # one dominant logit
    add(torch.full((V,), 1.5), V // 2)                                  # all equal
    r, j = rnd(), pick()
    r[torch.rand(V, generator=g) < 0.5] = NEG
    r[j] = 0.25
    add(r, j)                                                           # a scattered half banned
    r, j = torch.full((V,), NEG), pick()
    r[j] = -3.0
    add(r, j)                                                           # all but one banned: logprob 0, entropy 0
    if V > 1:
        r, j = rnd(), pick()
        r[j] = NEG
        add(r, j)                                                       # the chosen token is banned: -inf, entropy finite
    r = rnd() * 0.25 + torch.where(torch.rand(V, generator=g) < 0.5, 80.0, -80.0)
    add(r, pick())                                                      # +-80: the max subtraction matters
    add(rnd(), 0)
    add(rnd(), V - 1)                                                   # the chosen token at both ends
    return torch.stack(rows), torch.tensor(toks, dtype=torch.int64)


def row_bars(x, tok, temperature, want_lp, want_ent):
    """Per row, the derived bars of tests/bars.py (select_logprob_bar, select_entropy_bar), each capped at this file's earlier hand-set TOL."""
    cpu_lp, cpu_ent = reference(x, tok, temperature, dtype=torch.float32)
    y = (x / torch.tensor(temperature, dtype=torch.float32)).double()
    b_lp, b_ent = torch.full_like(want_lp, TOL), torch.full_like(want_ent, TOL)
    for r in range(x.shape[0]):
        fin = y[r][torch.isfinite(y[r])]
        if torch.isfinite(want_lp[r]):
            b_lp[r] = min(TOL, bars.select_logprob_bar(want_lp[r:r + 1], cpu_lp[r:r + 1], x.shape[1], sizes=(fin, fin - fin.max(), want_lp[r])))
        b_ent[r] = min(TOL, bars.select_entropy_bar(y[r:r + 1], want_ent[r:r + 1], cpu_ent[r:r + 1]))
    return b_lp, b_ent


def strided(x, ld, dev):
    """x [rows, V] on the device with row stride ld; the padding columns hold NaN, so a read past V poisons the result."""
    buf = torch.full((x.shape[0], ld), float("nan"), device=dev)
    buf[:, : x.shape[1]] = x.to(dev)
    return buf[:, : x.shape[1]]


def close(got, want, bar=None):
    """max |got - want| over the finite entries, each within its bar (where one is given); the infinite ones must agree exactly."""
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], want[inf].float()), (got, want)
    err = (got.double()[~inf] - want[~inf]).abs()
    assert bar is None or bool((err <= bar[~inf]).all()), (err, bar[~inf])
    return float(err.max()) if (~inf).any() else 0.0


@pytest.mark.parametrize("temperature", [1.0, 0.7, 2.5])
@pytest.mark.parametrize("V", VS)
def test_against_float64(dev, V, temperature):
    x, tok = pattern_rows(V, seed=V)
    want_lp, want_ent = reference(x, tok, temperature)
    P = x.shape[0]
    bar_lp, bar_ent = row_bars(x, tok, temperature, want_lp, want_ent)
    if V > 1:
        assert want_lp[5] == NEG and torch.isfinite(want_ent[5])
    assert abs(float(want_lp[4])) == 0.0 and abs(float(want_ent[4])) < 1e-12
    worst_lp = worst_ent = 0.0
    for rows in ([1, 3] if V > 100000 else [1, 3, 16, 33]):
        for ld in (V, V + 5):
            for start in range(0, P, rows):
                idx = torch.arange(start, start + rows) % P
                lp, ent = ops.row_scores(strided(x[idx], ld, dev), tok[idx].to(dev), temperature, entropy=True)
                only = ops.row_scores(strided(x[idx], ld, dev), tok[idx].to(dev), temperature)
                assert torch.equal(only.view(torch.int32), lp.view(torch.int32))            # entropy=False: the same logprob
                worst_lp = max(worst_lp, close(lp.cpu(), want_lp[idx], bar_lp[idx]))
                worst_ent = max(worst_ent, close(ent.cpu(), want_ent[idx], bar_ent[idx]))
                assert (ent >= 0).all()
    print(f"row_scores V={V} t={temperature}: max |dlogprob| {worst_lp:.2e}, max |dentropy| {worst_ent:.2e}")
    WORST["logprob"], WORST["entropy"] = max(WORST["logprob"], worst_lp), max(WORST["entropy"], worst_ent)
    print(f"row_scores so far: max |dlogprob| {WORST['logprob']:.2e}, max |dentropy| {WORST['entropy']:.2e}")
    assert worst_lp <= TOL and worst_ent <= TOL, (worst_lp, worst_ent)


def test_row_of_nothing_but_banned_tokens_is_nan(dev):
    x = torch.full((2, 1000), NEG, device=dev)
    x[1] = torch.randn(1000, device=dev)
    lp, ent = ops.row_scores(x, torch.tensor([3, 3], device=dev), entropy=True)
    assert torch.isnan(lp[0]) and torch.isnan(ent[0]) and torch.isfinite(lp[1]) and torch.isfinite(ent[1])


def test_without_tokens_is_minus_logsumexp(dev):
    x, _ = pattern_rows(4097, seed=3)
    for t in (1.0, 0.7):
        got = ops.row_scores(x.to(dev), None, t).cpu()
        want = -torch.logsumexp(x.double() / float(torch.tensor(t, dtype=torch.float32)), 1)
        assert (got.double() - want).abs().max() <= TOL


@pytest.mark.parametrize("V", [1000, 32000, 128256])
def test_repeats_bit_for_bit(dev, V):
    x, tok = pattern_rows(V, seed=V + 7)
    x, tok = x.to(dev), tok.to(dev)
    a = ops.row_scores(x, tok, 0.7, entropy=True)
    b = ops.row_scores(x, tok, 0.7, entropy=True)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    # a row's result does not depend on its neighbours
    one = ops.row_scores(x[3:4], tok[3:4], 0.7, entropy=True)
    assert torch.equal(one[0].view(torch.int32), a[0][3:4].view(torch.int32)) and torch.equal(one[1].view(torch.int32), a[1][3:4].view(torch.int32))


@pytest.mark.parametrize("V", [65, 4097, 128256])
def test_log_probability_rows(dev, V):
    """logprobs=True: the chosen entry comes back bit for bit (no normalisation, no temperature) and the entropy is -sum exp(x) * x."""
    g = torch.Generator().manual_seed(V)
    x = torch.log_softmax(torch.randn(5, V, generator=g) * 4, dim=1)
    x[1, torch.rand(V, generator=g) < 0.3] = NEG                       # banned after the log-softmax, as HF's processors do
    x[2] *= 1.3                                                         # a repetition penalty leaves rows that no longer sum to one
    tok = torch.randint(0, V, (5,), generator=g)
    x[3, tok[3]] = NEG
    for ld in (V, V + 5):
        xd = strided(x, ld, dev)
        lp, ent = ops.row_scores(xd, tok.to(dev), 0.5, entropy=True, logprobs=True)
        assert torch.equal(lp.cpu().view(torch.int32), x.gather(1, tok[:, None])[:, 0].view(torch.int32))
        xd64 = x.double()
        want = -torch.where(torch.isinf(xd64), torch.zeros_like(xd64), torch.exp(xd64) * xd64).sum(1)
        assert (ent.cpu().double() - want).abs().max() <= TOL
        assert torch.equal(ops.row_scores(xd, tok.to(dev), logprobs=True).view(torch.int32), lp.view(torch.int32))


def test_tokens_out_of_range_are_clamped(dev):
    x = torch.randn(2, 100, device=dev)
    got = ops.row_scores(x, torch.tensor([-5, 1000], device=dev))
    want = ops.row_scores(x, torch.tensor([0, 99], device=dev))
    assert torch.equal(got, want)


def test_bad_arguments(dev):
    x = torch.randn(4, 256, device=dev)
    tok = torch.zeros(4, dtype=torch.int64, device=dev)
    for bad_x, bad_t in ((x.bfloat16(), tok), (x[0], tok[:1]), (x, tok.int()), (x, tok[:3]), (x.t(), torch.zeros(256, dtype=torch.int64, device=dev)),
                         (x.cpu(), tok)):
        with pytest.raises((ValueError, L.AvllmError)):
            ops.row_scores(bad_x, bad_t)
    with pytest.raises(L.AvllmError, match="float32"):
        ops.row_scores(x.bfloat16(), tok)
    for t in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.row_scores(x, tok, t)
    lib = L.load()
    out = torch.empty(4, device=dev)
    assert lib.avllm_row_scores(L.ptr(x), 256, 4, 256, L.ptr(tok), 1.0, None, None, L.F32, L.stream_ptr()) == 1       # no output at all
    assert lib.avllm_row_scores(L.ptr(x), 100, 4, 256, L.ptr(tok), 1.0, L.ptr(out), None, L.F32, L.stream_ptr()) == 1  # ld < V
    assert math.isfinite(float(ops.row_scores(x, tok)[0]))
