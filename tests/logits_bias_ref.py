"""`chain`: a plain-torch fp32 restatement of the seven logits processors generate() has, in GenerationMixin._get_logits_processor's order
(sequence bias, repetition penalty, no-repeat n-gram, bad words, min-new-tokens, suppress, begin-suppress), and `cases`, the seeded case
list tests/test_logits_bias_cpu.py holds it to transformers' own classes on and tests/test_logits_bias_gpu.py holds the kernel to it on.
The three older processors are test_logits_process_cpu.restate."""
import torch

from test_logits_process_cpu import ALPHABET, EOS, NEG_INF, make, restate

# last tokens of the constructed sequences; outside ALPHABET, so only the sequence bias touches them
SHARED, OTHER = 5, 7


def add_sequence_bias(s, hist, seqs):
    """SequenceBiasLogitsProcessor: seqs {tuple of ids: bias}.  One fp32 bias per (row, token), accumulated from +0: the length-1 entry,
    then in the dict's order every longer sequence of L <= n tokens (n = hist.shape[1]; HF's test, not L - 1 <= n) whose first L - 1
    tokens are the row's last L - 1; then added to the scores once, everywhere (as HF adds its whole bias tensor)."""
    rows, n = hist.shape
    bias = torch.zeros_like(s)
    for q, b in seqs.items():
        if len(q) == 1:
            bias[:, q[0]] += torch.tensor(b, dtype=torch.float32)
    for q, b in seqs.items():
        if len(q) == 1 or len(q) > n:
            continue
        for r in range(rows):
            if hist[r, n - (len(q) - 1):].tolist() == list(q[:-1]):
                bias[r, q[-1]] += torch.tensor(b, dtype=torch.float32)
    return s + bias


def chain(scores, hist, sequence_bias=None, p=1.0, ngram=0, bad_words_ids=None, m=0, eos=None, suppress_tokens=None,
          begin_suppress_tokens=None, log_softmax=False, stage_dtype=None):
    """scores [rows, V], hist int64 [rows, n] -> processed fp32 scores.  log_softmax: beam search's order, the processors on the
    log-probabilities.  stage_dtype (bf16 scores): each arithmetic stage computes in fp32 on the stored value and rounds once."""
    rnd = (lambda t: t.to(stage_dtype).float()) if stage_dtype is not None else (lambda t: t)
    s = scores.float().clone()
    if log_softmax:
        s = torch.log_softmax(s, dim=-1)
    if sequence_bias:
        s = rnd(add_sequence_bias(s, hist, sequence_bias))
    s = rnd(restate(s, hist, p, ngram, 0, None))
    if bad_words_ids:
        banned = {tuple(w): NEG_INF for w in bad_words_ids if eos is None or list(w) != [eos]}       # HF's constructor drops [eos]
        s = add_sequence_bias(s, hist, banned)
    s = restate(s, hist, 1.0, 0, m, eos)
    if suppress_tokens:
        s[:, sorted(set(suppress_tokens))] = NEG_INF
    if begin_suppress_tokens and hist.shape[1] == 0:
        s[:, sorted(set(begin_suppress_tokens))] = NEG_INF
    return s


def make_case(V, n, with_len1, old, log_softmax, rows=3):
    """One case: histories over the five-token ALPHABET (so rows share tails and tokens repeat), sequences cut from the rows' own tails.
      * three sequences of 2, 3 and 4 tokens ending in SHARED whose prefixes are row 0's last 1, 2 and 3 tokens (where it has them), listed
        in the order 3, 2, 4 with biases 0.1, 3e7, -3e7: fp32 addition in another order gives another total; at n = L - 1 the prefix is
        there but HF's L <= n test is not met, at n = L it is;
      * with_len1: a length-1 entry on SHARED too, listed last, accumulated first;
      * a 2-token sequence on row 1's last token ending in OTHER, and one whose prefix is not in the alphabet;
      * a length-1 entry on row 0's first history token whose bias flips the sign of row 0's score there (the penalty of the `old`
        settings then multiplies where it would have divided, or the reverse);
      * bad words: [EOS] (dropped), a single token, and row 0's last token followed by 9; a suppress list with duplicates; a begin list."""
    scores, hist = make(V, n, seed=1000 * V + 10 * n + with_len1, rows=rows)
    sb = {}
    for L, b in ((3, 0.1), (2, 3e7), (4, -3e7)):
        if L - 1 <= n:
            sb[tuple(hist[0, n - (L - 1):].tolist()) + (SHARED,)] = b
    if n >= 1 and rows > 1:
        sb[(int(hist[1, n - 1]), OTHER)] = -2.5
    sb[(8, 9, OTHER)] = 4.0
    if n >= 1:
        t = int(hist[0, 0])
        sb[(t,)] = -2.0 * float(scores[0, t])
    if with_len1:
        sb[(SHARED,)] = 0.25
    bad = [[EOS], [11]]
    if n >= 1:
        bad.append([int(hist[0, n - 1]), 9])
    p, ngram, m = (1.3, 2, n + 1) if old else (1.0, 0, 0)
    return dict(scores=scores, hist=hist, sequence_bias=sb, p=p, ngram=ngram, bad_words_ids=bad, m=m, eos=EOS,
                suppress_tokens=[2, 2, 13, 96, 13], begin_suppress_tokens=[4, 17, 4], log_softmax=log_softmax)


def cases():
    for V in (97, 1000):
        for n in range(7):
            for with_len1 in (False, True):
                for old in (False, True):
                    for log_softmax in (False, True):
                        yield make_case(V, n, with_len1, old, log_softmax)


def knobs(case):
    return {k: v for k, v in case.items() if k not in ("scores", "hist")}
