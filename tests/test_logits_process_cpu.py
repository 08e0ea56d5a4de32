"""CPU: `restate`, the restatement of HF's RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor
that tests/test_logits_process_gpu.py and tests/test_generate_processors_gpu.py hold the device kernel to, against HF's own three classes
(where transformers imports), and the argument rules of ops.check_logits_processors."""
import pytest
import torch

from avllm import ops

NEG_INF = float("-inf")
ALPHABET = torch.tensor([3, 17, 42, 64, 96])          # histories draw from five tokens: duplicates and repeated n-grams are dense
EOS = 17                                             # in the alphabet, so the penalty, the ban and min_new_tokens meet on one entry
VOCABS = [97, 32000, 128256]
PENALTIES = [0.5, 1.3]
NGRAMS = [0, 1, 2, 4]


def restate(scores, hist, p, n, m, eos):
    """scores [rows, V] (CPU), hist [rows, cur] int64: the three processors in HF's order.  The penalty is gathered from the unprocessed
    scores and scattered once, so a token that occurs several times is penalised once."""
    s = scores.clone()
    cur = hist.shape[1]
    if p != 1.0 and cur:
        g = torch.gather(s, 1, hist)
        s = s.scatter(1, hist, torch.where(g < 0, g * p, g / p))
    if n > 0 and cur + 1 >= n:
        for r in range(hist.shape[0]):
            h = hist[r].tolist()
            prefix = h[cur + 1 - n:]
            banned = [h[i + n - 1] for i in range(cur - n + 1) if h[i:i + n - 1] == prefix]
            if banned:
                s[r, banned] = NEG_INF
    if eos is not None and cur < m:
        s[:, eos] = NEG_INF
    return s


def hf_chain(scores, hist, p, n, m, eos):
    from transformers.generation import logits_process as LP
    s = scores.clone()
    if p != 1.0:
        s = LP.RepetitionPenaltyLogitsProcessor(penalty=p)(hist, s)
    if n > 0:
        s = LP.NoRepeatNGramLogitsProcessor(n)(hist, s)
    if eos is not None and m > 0:
        s = LP.MinNewTokensLengthLogitsProcessor(0, m, eos, device="cpu")(hist, s)
    return s


def lengths(n):
    return sorted({c for c in (0, 1, n - 2, n - 1, 300, 1024) if c >= 0})


def make(V, cur, seed, rows=3):
    g = torch.Generator().manual_seed(seed)
    scores = torch.randn(rows, V, generator=g) * 4
    hist = ALPHABET[torch.randint(0, len(ALPHABET), (rows, cur), generator=g)]
    return scores, hist


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("p", PENALTIES)
def test_restatement_matches_transformers(p):
    pytest.importorskip("transformers")
    for V in VOCABS:
        for n in NGRAMS:
            for cur in lengths(n):
                for m in (cur, cur + 1):
                    scores, hist = make(V, cur, seed=V + 31 * n + cur)
                    want = hf_chain(scores, hist, p, n, m, EOS)
                    got = restate(scores, hist, p, n, m, EOS)
                    assert same_bits(got, want), (V, p, n, cur, m)


def test_argument_rules():
    """HF's: a strictly positive float penalty, non-negative integers for the other two; no GPU needed to refuse."""
    for bad in (0, -1, "x", None, float("inf")):
        with pytest.raises(ValueError):
            ops.check_logits_processors(bad, 0, 0)
    for bad in (-1, 1.5, "2"):
        with pytest.raises(ValueError):
            ops.check_logits_processors(1.0, bad, 0)
        with pytest.raises(ValueError):
            ops.check_logits_processors(1.0, 0, bad)
    assert ops.check_logits_processors(1.0, 0, 0) is False
    assert ops.check_logits_processors(1, 0, 0) is False
    assert all(ops.check_logits_processors(*a) for a in ((1.2, 0, 0), (1.0, 3, 0), (1.0, 0, 5), (0.5, 1, 1)))
