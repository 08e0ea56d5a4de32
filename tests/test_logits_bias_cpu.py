"""CPU: logits_bias_ref.chain, the restatement tests/test_logits_bias_gpu.py and tests/test_generate_bias_gpu.py hold the device to, against
transformers' own processor objects in GenerationMixin._get_logits_processor's order; the argument rules of ops.check_logits_bias; the
hotword expansion of generate(hotwords=); and the avllm_logits_proc_desc layout against its ctypes mirror."""
import ctypes
import os
import subprocess

import pytest
import torch

from avllm import lib as L
from avllm import ops
from avllm.model import hotword_sequence_bias
from avllm.tokenizer import ByteTokenizer
from logits_bias_ref import SHARED, cases, chain, knobs
from test_logits_process_cpu import EOS, NEG_INF, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hf_chain(scores, hist, sequence_bias, p, ngram, bad_words_ids, m, eos, suppress_tokens, begin_suppress_tokens, log_softmax):
    """transformers' processors as _get_logits_processor appends them; with inputs_embeds the prompt length (and so begin_index) is 0."""
    from transformers.generation import logits_process as LP
    s = torch.log_softmax(scores, dim=-1) if log_softmax else scores.clone()
    procs = []
    if sequence_bias is not None:
        procs.append(LP.SequenceBiasLogitsProcessor(sequence_bias=dict(sequence_bias)))
    if p != 1.0:
        procs.append(LP.RepetitionPenaltyLogitsProcessor(penalty=p))
    if ngram > 0:
        procs.append(LP.NoRepeatNGramLogitsProcessor(ngram))
    if bad_words_ids is not None:
        procs.append(LP.NoBadWordsLogitsProcessor(bad_words_ids, torch.tensor([eos])))
    if m > 0:
        procs.append(LP.MinNewTokensLengthLogitsProcessor(0, m, torch.tensor([eos]), device="cpu"))
    if suppress_tokens is not None:
        procs.append(LP.SuppressTokensLogitsProcessor(suppress_tokens, device="cpu"))
    if begin_suppress_tokens is not None:
        procs.append(LP.SuppressTokensAtBeginLogitsProcessor(begin_suppress_tokens, 0, device="cpu"))
    for proc in procs:
        s = proc(hist, s)
    return s


def test_restatement_matches_transformers():
    pytest.importorskip("transformers")
    checked = acted = 0
    for c in cases():
        want = hf_chain(c["scores"], c["hist"], **knobs(c))
        got = chain(c["scores"], c["hist"], **knobs(c))
        assert same_bits(got, want), (c["scores"].shape, c["hist"].shape, knobs(c), (got != want).nonzero()[:5])
        plain = torch.log_softmax(c["scores"], dim=-1) if c["log_softmax"] else c["scores"]
        acted += int((got[:, SHARED] != plain[:, SHARED]).any())
        checked += 1
    assert checked == 2 * 7 * 2 * 2 * 2 and acted >= checked // 2


def test_each_processor_alone_matches_transformers():
    pytest.importorskip("transformers")
    off = dict(sequence_bias=None, p=1.0, ngram=0, bad_words_ids=None, m=0, eos=EOS, suppress_tokens=None, begin_suppress_tokens=None,
               log_softmax=False)
    for c in cases():
        for name in ("sequence_bias", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens"):
            kw = dict(off, **{name: c[name]})
            assert same_bits(chain(c["scores"], c["hist"], **kw), hf_chain(c["scores"], c["hist"], **kw)), (name, c["hist"].shape)


def test_the_l_le_n_rule_and_begin_index():
    """HF's quirk: a sequence of L tokens is considered from n = L generated tokens on, although its prefix has only L - 1; begin-suppress acts
    at n = 0 only."""
    s = torch.zeros(1, 97)
    sb = {(3, 5): 2.0}
    assert chain(s, torch.tensor([[3]]), sequence_bias=sb)[0, 5] == 0.0           # n = 1 = L - 1: prefix there, not applied
    assert chain(s, torch.tensor([[4, 3]]), sequence_bias=sb)[0, 5] == 2.0        # n = 2 = L
    assert chain(s, torch.zeros(1, 0, dtype=torch.int64), begin_suppress_tokens=[4])[0, 4] == NEG_INF
    assert chain(s, torch.tensor([[3]]), begin_suppress_tokens=[4])[0, 4] == 0.0


def test_argument_rules():
    ok = dict(sequence_bias={(1, 2): 1.0, (3,): -2.0}, bad_words_ids=[[4, 5], [6]], suppress_tokens=[1, 1, 2], begin_suppress_tokens=[0])
    assert ops.check_logits_bias(**ok, vocab=97, eos=2) is True
    assert ops.check_logits_bias() is False
    assert ops.check_logits_bias(suppress_tokens=[]) is False
    assert ops.check_logits_bias(sequence_bias=[[[1, 2], 1.0]], vocab=97) is True
    bad = [
        dict(sequence_bias={}), dict(sequence_bias=[]), dict(sequence_bias="x"), dict(sequence_bias={(): 1.0}), dict(sequence_bias={(1, -2): 1.0}),
        dict(sequence_bias={(1, 2.5): 1.0}), dict(sequence_bias={(1, True): 1.0}), dict(sequence_bias={(1,): 1}), dict(sequence_bias={(1,): "a"}),
        dict(sequence_bias={(1,): float("inf")}), dict(sequence_bias={(1,): float("nan")}), dict(sequence_bias={1: 1.0}),
        dict(sequence_bias={(97,): 1.0}), dict(sequence_bias=[[[1, 2]]]), dict(sequence_bias=[[[], 1.0]]),
        dict(bad_words_ids=[]), dict(bad_words_ids=[[]]), dict(bad_words_ids=[3]), dict(bad_words_ids=[[1, -1]]), dict(bad_words_ids=[[1.0]]),
        dict(bad_words_ids=[[97]]), dict(bad_words_ids=[[2]]), dict(bad_words_ids="ab"),
        dict(suppress_tokens=[-1]), dict(suppress_tokens=[1.5]), dict(suppress_tokens=[97]), dict(suppress_tokens="12"), dict(suppress_tokens=3),
        dict(begin_suppress_tokens=[-1]), dict(begin_suppress_tokens=[True]), dict(begin_suppress_tokens=[97]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.check_logits_bias(**kw, vocab=97, eos=2)
    # the capacities, refused by name
    assert ops.LOGITS_BIAS_MAX_SEQUENCES >= 1024 and ops.LOGITS_BIAS_MAX_SEQUENCE_LENGTH >= 16
    many = {(i % 90, i // 90): 1.0 for i in range(ops.LOGITS_BIAS_MAX_SEQUENCES + 1)}
    with pytest.raises(ValueError, match="LOGITS_BIAS_MAX_SEQUENCES"):
        ops.check_logits_bias(sequence_bias=many, vocab=97)
    with pytest.raises(ValueError, match="LOGITS_BIAS_MAX_SEQUENCES"):
        ops.check_logits_bias(bad_words_ids=[list(k) for k in many], vocab=97)
    long = tuple(range(ops.LOGITS_BIAS_MAX_SEQUENCE_LENGTH + 1))
    with pytest.raises(ValueError, match="LOGITS_BIAS_MAX_SEQUENCE_LENGTH"):
        ops.check_logits_bias(sequence_bias={long: 1.0}, vocab=97)
    with pytest.raises(ValueError, match="LOGITS_BIAS_MAX_SEQUENCE_LENGTH"):
        ops.check_logits_bias(bad_words_ids=[list(long)], vocab=97)
    assert ops.check_logits_bias(sequence_bias={long[:-1]: 1.0}, suppress_tokens=list(range(97)), vocab=97)


def test_hotword_expansion():
    tok = ByteTokenizer(512)
    ids = lambda text: tuple(b + 3 for b in text.encode())  # noqa: E731
    got = hotword_sequence_bias(tok, ["ab", "ac"], 2.5)
    want = [ids("a"), ids("ab"), ids(" "), ids(" a"), ids(" ab"), ids("ac"), ids(" ac")]       # every prefix, shared ones merged
    assert list(got) == want and set(got.values()) == {2.5}
    # the user's entries come first and stay; the forms [[ids, bias]] and {ids: bias} are both taken
    user = {ids("zz"): -1.0}
    both = hotword_sequence_bias(tok, ["ab"], 2.5, user)
    assert list(both)[0] == ids("zz") and both[ids("zz")] == -1.0 and both[ids(" ab")] == 2.5
    assert hotword_sequence_bias(tok, ["ab"], 2.5, [[list(ids("zz")), -1.0]]) == both
    assert hotword_sequence_bias(tok, [" ab "], 2.5) == hotword_sequence_bias(tok, ["ab"], 2.5)
    for clash in ({ids("a"): 1.0}, {ids(" ab"): 1.0}):
        with pytest.raises(ValueError, match="sequence_bias key"):
            hotword_sequence_bias(tok, ["ab"], 2.5, clash)
    for bad_words, bias in (("ab", 1.0), ([""], 1.0), ([3], 1.0), (["ab"], float("nan")), (["ab"], "x"), (["ab"], None)):
        with pytest.raises(ValueError):
            hotword_sequence_bias(tok, bad_words, bias)
    ops.check_logits_bias(sequence_bias=got, vocab=512)
    with pytest.raises(ValueError, match="LOGITS_BIAS_MAX_SEQUENCE_LENGTH"):                    # a word longer than a table entry
        ops.check_logits_bias(sequence_bias=hotword_sequence_bias(tok, ["a" * 17], 1.0), vocab=512)


def test_descriptor_layout_matches_header(tmp_path):
    """sizeof and every offsetof of avllm_logits_proc_desc against lib.LogitsProcDesc, and the two capacities, via a probe compiled with gcc."""
    names = [n for n, _ in L.LogitsProcDesc._fields_]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "avllm.h"\nint main(){printf("%zu %d %d", sizeof(avllm_logits_proc_desc), ' \
           'AVLLM_LOGITS_MAX_SEQUENCES, AVLLM_LOGITS_MAX_SEQUENCE_LEN);\n' + \
           "".join(f'printf(" %zu", offsetof(avllm_logits_proc_desc, {n}));\n' for n in names) + "return 0;}\n"
    c, exe = tmp_path / "p.c", tmp_path / "p"
    c.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert out[0] == ctypes.sizeof(L.LogitsProcDesc)
    assert out[1:3] == [ops.LOGITS_BIAS_MAX_SEQUENCES, ops.LOGITS_BIAS_MAX_SEQUENCE_LENGTH]
    assert out[3:] == [getattr(L.LogitsProcDesc, n).offset for n in names]
    assert "avllm_logits_process_ex" in L.EXPORTS
