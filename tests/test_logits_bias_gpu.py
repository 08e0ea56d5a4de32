"""ops.logits_process with the sequence-bias, bad-words, suppress and begin-suppress tables (csrc/logits_process.hip,
avllm_logits_process_ex) against logits_bias_ref.chain, the CPU restatement of HF's seven processors (itself held to transformers' classes
in tests/test_logits_bias_cpu.py), bit for bit: f32 and bf16 scores, 1 to 3 rows, a row stride larger than V, the history length as an int
and in device memory, `append`, the log-softmax mode of beam search, every table alone, tables larger than a workgroup, and the refusals."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402
from logits_bias_ref import chain, knobs, make_case  # noqa: E402
from test_logits_process_cpu import ALPHABET, EOS, make, restate, same_bits  # noqa: E402

TABLE_NAMES = ("sequence_bias", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens")
PAD_L, PAD_R = 5, 72


def tables_of(c, V, only=None):
    kw = {k: c[k] for k in TABLE_NAMES if only is None or k == only}
    return ops.logits_bias_tables(**kw, vocab=V, eos=c["eos"])


def launch(scores, hist, c, tables, cur_dev=False, append=False, strided=False, log_softmax=None):
    """The kernel on device copies.  The history tensor is wider than n (entries past n must not be read); strided: the rows sit inside a
    wider buffer, whose margins are returned too; append: the last token arrives in a [rows] tensor and must be stored by the launch."""
    rows, V = scores.shape
    n = hist.shape[1]
    wide = torch.full((rows, max(n + 5, 8)), int(ALPHABET[0]), dtype=torch.int64)
    wide[:, :n] = hist
    app = None
    if append and n:
        wide[:, n - 1] = 0
        app = hist[:, n - 1].contiguous().cuda()
    buf = torch.zeros(rows, PAD_L + V + PAD_R, dtype=scores.dtype) if strided else scores.clone()
    view = buf[:, PAD_L:PAD_L + V] if strided else buf
    view.copy_(scores)
    d_buf = buf.cuda()
    d_view = d_buf[:, PAD_L:PAD_L + V] if strided else d_buf
    d_hist = wide.cuda()
    cur = torch.tensor([n], dtype=torch.int32, device="cuda") if cur_dev else n
    ops.logits_process(d_view, d_hist, cur, c["p"], c["ngram"], c["m"], eos=c["eos"], append=app,
                       log_softmax=c["log_softmax"] if log_softmax is None else log_softmax, **tables)
    if app is not None:
        assert torch.equal(d_hist.cpu()[:, :n], hist)
    out = d_buf.cpu()
    if strided:
        assert (out[:, :PAD_L] == 0).all() and (out[:, PAD_L + V:] == 0).all(), "the margins of a strided buffer were written"
        out = out[:, PAD_L:PAD_L + V]
    return out


def all_cases():
    i = 0
    for V in (97, 1000):
        for n in range(7):
            for with_len1 in (False, True):
                for old in (False, True):
                    for log_softmax in (False, True):
                        yield i, V, make_case(V, n, with_len1, old, log_softmax, rows=1 + i % 3)
                        i += 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_matches_restatement_bit_for_bit(dev, dtype):
    checked = 0
    for i, V, c in all_cases():
        if c["log_softmax"] and dtype != torch.float32:          # the log-softmax mode takes f32 rows
            continue
        scores, hist = c["scores"].to(dtype), c["hist"]
        form = dict(cur_dev=bool(i & 1), append=bool(i & 2), strided=bool(i & 4))
        tb = tables_of(c, V)
        if c["log_softmax"]:
            # the kernel's own log-softmax (its sum order differs from torch's; pinned in test_logits_process_gpu), then the chain on it
            off = dict(c, p=1.0, ngram=0, m=0)
            own = launch(scores, hist, off, {}, log_softmax=True)
            want = chain(own, hist, **dict(knobs(c), log_softmax=False))
        elif dtype == torch.float32:
            want = chain(scores, hist, **knobs(c))
        else:
            want = chain(scores, hist, **knobs(c), stage_dtype=dtype).to(dtype)
        got = launch(scores, hist, c, tb, **form)
        bits = (lambda t: t.view(torch.int32)) if dtype == torch.float32 else (lambda t: t.view(torch.int16))
        assert torch.equal(bits(got), bits(want)), (i, V, hist.shape, form, knobs(c), (bits(got) != bits(want)).nonzero()[:5])
        again = launch(scores, hist, c, tb, **form)
        assert torch.equal(bits(again), bits(got)), "two launches must give identical bits"
        checked += 1
    assert checked == (112 if dtype == torch.float32 else 56)


def test_each_table_alone_and_none_is_the_old_entry(dev):
    V = 1000
    for n in (0, 1, 4):
        c = make_case(V, n, True, False, False)
        scores, hist = c["scores"], c["hist"]
        off = dict(sequence_bias=None, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None)
        for name in TABLE_NAMES:
            tb = tables_of(c, V, only=name)
            assert list(tb) == [name]
            want = chain(scores, hist, **dict(knobs(c), **dict(off, **{name: c[name]})))
            assert same_bits(launch(scores, hist, c, tb), want), (n, name)
            assert same_bits(want, scores) == (name == "begin_suppress_tokens" and n > 0), (n, name)
        # every table None: the old entry's result, with and without the older processors
        for p, g, m in ((1.0, 0, 0), (1.3, 2, n + 1)):
            old = dict(c, p=p, ngram=g, m=m)
            got = launch(scores, hist, old, dict(off))
            assert same_bits(got, restate(scores, hist, p, g, m, EOS))
    # the library entry itself with empty tables: what avllm_logits_process does with the same arguments
    scores, hist = make(V, 4, seed=3)
    a, b, h = scores.cuda(), scores.cuda(), hist.cuda()
    ops.logits_process(a, h, 4, 1.3, 2, 5, eos=EOS)
    d = L.LogitsProcDesc(scores=b.data_ptr(), ld=V, rows=3, V=V, dtype=L.F32, history=h.data_ptr(), ldh=4, cur=4, repetition_penalty=1.3,
                         no_repeat_ngram_size=2, min_new_tokens=5, eos=EOS)
    L.check(L.load().avllm_logits_process_ex(ctypes.byref(d), L.stream_ptr()))
    assert same_bits(a.cpu(), b.cpu()) and not same_bits(a.cpu(), scores)
    d.repetition_penalty, d.no_repeat_ngram_size, d.min_new_tokens = 1.0, 0, 0               # everything off: nothing is written
    c2 = scores.cuda()
    d.scores = c2.data_ptr()
    L.check(L.load().avllm_logits_process_ex(ctypes.byref(d), L.stream_ptr()))
    assert same_bits(c2.cpu(), scores)


def test_tables_larger_than_a_workgroup_and_a_full_vocabulary_list(dev):
    """1500 entries per sequence table (a thread owns more than one; groups of one last token are ~150 entries long and one of them spans
    the 1024-entry stride), and a suppress list of all but 100 ids at V = 151936."""
    V, n, rows = 151936, 40, 2
    g = torch.Generator().manual_seed(7)
    scores, hist = make(V, n, seed=11, rows=rows)
    lasts = [100 + 7 * j for j in range(10)]
    sb, bad = {}, []
    rnd = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))  # noqa: E731
    while len(sb) < 1500:
        Lq = rnd(1, 5)
        # prefixes: a row's own tail (the entry applies), or that tail with one token replaced (it does not)
        pre = hist[rnd(0, rows), n - (Lq - 1):].tolist() if Lq > 1 else []
        if pre and rnd(0, 4):
            pre[rnd(0, len(pre))] = rnd(0, V)
        last = lasts[rnd(0, 10)] if Lq > 1 or rnd(0, 2) else 20000 + len(sb)
        sb[tuple(pre) + (last,)] = float(torch.randn(1, generator=g)) * 10.0 ** rnd(-2, 7)
    for j, q in enumerate(sb):
        bad.append(list(q[:-1]) + [200000 % V + j])
    allowed = set(range(1000, 1100))
    c = dict(sequence_bias=sb, p=1.3, ngram=2, bad_words_ids=bad, m=0, eos=EOS, suppress_tokens=[t for t in range(V) if t not in allowed],
             begin_suppress_tokens=None, log_softmax=False)
    tb = ops.logits_bias_tables(sb, bad, c["suppress_tokens"], None, vocab=V, eos=EOS)
    assert tb["sequence_bias"].n == 1500 and tb["bad_words_ids"].n == 1500 and tb["suppress_tokens"].n == V - 100
    # without the suppress list (which leaves 100 finite entries), then with it
    for sup in (None, c["suppress_tokens"]):
        cc = dict(c, suppress_tokens=sup)
        t2 = {k: v for k, v in tb.items() if sup is not None or k != "suppress_tokens"}
        want = chain(scores, hist, **cc)
        got = launch(scores, hist, cc, t2, strided=True)
        assert same_bits(got, want), (got != want).nonzero()[:5]
        assert same_bits(launch(scores, hist, cc, t2, strided=True), got)
    assert torch.isfinite(got).sum() <= 100 * rows


def test_single_token_tables_need_no_history(dev):
    """Only multi-token sequences and the older processors read the history: with single-token tables it may be None and the 1024-token
    limit does not apply; begin-suppress still tells n = 0 from n > 0, also with n in device memory."""
    V = 97
    scores, _ = make(V, 0, seed=5)
    tb = ops.logits_bias_tables({(5,): 1.5, (9,): -2.0}, [[11]], [2, 13], [4], vocab=V, eos=EOS)
    kw = dict(sequence_bias={(5,): 1.5, (9,): -2.0}, bad_words_ids=[[11]], suppress_tokens=[2, 13], begin_suppress_tokens=[4])
    for n in (0, 1, 5000):
        want = chain(scores, torch.zeros(3, min(n, 1), dtype=torch.int64), **kw)
        for cur in (n, torch.tensor([n], dtype=torch.int32, device="cuda")):
            got = ops.logits_process(scores.cuda(), None, cur, **tb).cpu()
            assert same_bits(got, want), n
    assert want[0, 4] == scores[0, 4]


def test_refusals(dev):
    V = 97
    scores = torch.zeros(2, V, device="cuda")
    hist = torch.zeros(2, 8, dtype=torch.int64, device="cuda")
    multi = ops.logits_bias_tables({(3, 5): 1.0}, vocab=V)
    multi_bad = ops.logits_bias_tables(bad_words_ids=[[3, 5]], vocab=V)
    single = ops.logits_bias_tables(suppress_tokens=[3], vocab=V)
    with pytest.raises(ValueError, match="prepared"):             # raw arguments are not tables
        ops.logits_process(scores, hist, 0, sequence_bias={(3, 5): 1.0})
    with pytest.raises(ValueError, match="prepared"):
        ops.logits_process(scores, hist, 0, suppress_tokens=[3])
    with pytest.raises(ValueError, match="prepared"):
        ops.logits_process(scores, hist, 0, suppress_tokens=multi["sequence_bias"])
    with pytest.raises(ValueError, match="vocabulary"):           # a table built for another V
        ops.logits_process(scores, hist, 0, **ops.logits_bias_tables(suppress_tokens=[3], vocab=V + 1))
    for tb in (multi, multi_bad):                                 # a multi-token sequence needs the history, within its limit
        with pytest.raises(ValueError, match="history"):
            ops.logits_process(scores, None, 3, **tb)
        big = torch.zeros(2, ops.LOGITS_PROCESS_MAX_HISTORY + 1, dtype=torch.int64, device="cuda")
        with pytest.raises(ValueError, match="at most"):
            ops.logits_process(scores, big, ops.LOGITS_PROCESS_MAX_HISTORY + 1, **tb)
        with pytest.raises(ValueError, match="at most"):
            ops.logits_process(scores, big, torch.zeros(1, dtype=torch.int32, device="cuda"), **tb)
        with pytest.raises(ValueError):
            ops.logits_process(scores, hist, 9, **tb)
    with pytest.raises(ValueError):                               # the older processors' rules still hold
        ops.logits_process(scores, hist, 0, 0.0, **single)
    with pytest.raises(ValueError, match="history"):
        ops.logits_process(scores, None, 1, 1.3, **single)
    with pytest.raises(ValueError, match="f32"):
        ops.logits_process(scores.bfloat16(), hist, 0, log_softmax=True, **single)
    for kw in (dict(sequence_bias={(V,): 1.0}), dict(bad_words_ids=[[V]]), dict(suppress_tokens=[V]), dict(begin_suppress_tokens=[-1]),
               dict(sequence_bias={(): 1.0}), dict(sequence_bias={(1,): float("inf")}), dict(bad_words_ids=[[EOS]])):
        with pytest.raises(ValueError):
            ops.logits_bias_tables(**kw, vocab=V, eos=EOS)
    # the library's own capacity checks, on tables that did not come from logits_bias_tables
    n = ops.LOGITS_BIAS_MAX_SEQUENCES + 1
    tok = torch.zeros(n, ops.LOGITS_BIAS_MAX_SEQUENCE_LENGTH, dtype=torch.int32, device="cuda")
    one = torch.ones(n, dtype=torch.int32, device="cuda")
    val = torch.zeros(n, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="at most"):
        ops.logits_process(scores, hist, 0, sequence_bias=ops.SequenceTable(tok, one, val, n, 1, V))
    with pytest.raises(ValueError, match="at most"):
        ops.logits_process(scores, hist, 0, bad_words_ids=ops.SequenceTable(tok, one, None, n, 1, V))
    with pytest.raises(ValueError, match="tokens"):
        ops.logits_process(scores, hist, 0, sequence_bias=ops.SequenceTable(tok, one, val, 4, ops.LOGITS_BIAS_MAX_SEQUENCE_LENGTH + 1, V))
    ids = torch.zeros(V + 1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="at most"):
        ops.logits_process(scores, hist, 0, suppress_tokens=ops.TokenTable(ids, V + 1, V))
    with pytest.raises(ValueError, match="at most"):
        ops.logits_process(scores, hist, 0, begin_suppress_tokens=ops.TokenTable(ids, V + 1, V))
    assert (scores == 0).all()
