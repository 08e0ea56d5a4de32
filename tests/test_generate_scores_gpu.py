"""generate(return_token_scores=True, num_return_sequences=n) on the tiny golden model: token log-probabilities and entropies of greedy,
sampled and beam-search decoding against transformers' compute_transition_scores (fp32, adapters off on both sides), the beam scorer's own
sums (fp32 and bf16), teacher forcing (bf16), and the n-best / repeated-draw layouts."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from avllm import ops  # noqa: E402
from avllm.model import GenerateOutput  # noqa: E402
from bars import BF16_LOGIT_MAX_ABS  # noqa: E402
from test_generate_beam_gpu import embeds, gen, with_eos  # noqa: E402,F401
from test_generate_processors_gpu import model16  # noqa: E402
from test_model_gpu import make_model, tiny  # noqa: E402,F401

N_NEW = 10
PROC = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, bad_words_ids=[[7]])


def scored(m, audio, video, dev, **kw):
    out = m.generate(audio=audio.to(dev), video=video.to(dev), max_new_tokens=kw.pop("max_new_tokens", N_NEW), return_token_scores=True, **kw)
    assert isinstance(out, GenerateOutput)
    return GenerateOutput(*(None if t is None else t.cpu() for t in out))


def lengths(ids, eos):
    """Tokens of each row up to and including its first eos (the whole row without one)."""
    L = ids.shape[1]
    return torch.tensor([row.index(eos) + 1 if eos in row else L for row in ids.tolist()])


def assert_masked(out, n):
    for r in range(out.sequences.shape[0]):
        assert (out.token_scores[r, n[r]:] == 0.0).all() and (out.token_entropy[r, n[r]:] == 0.0).all(), (r, out)


@pytest.fixture(scope="module")
def m32(dev, tiny):  # noqa: F811
    g, oc, W, *_ = tiny
    return make_model(oc, W, "fp32", max_seq_len=256).eval()


@pytest.fixture(scope="module")
def m16(dev, tiny):  # noqa: F811
    g, oc, W, *_ = tiny
    return make_model(oc, W, "bf16", max_seq_len=256).eval()


@pytest.fixture(scope="module")
def hf_llm(tiny):  # noqa: F811
    tf = pytest.importorskip("transformers")
    g, oc, W, *_ = tiny
    lc = oc.llama
    llm = tf.LlamaForCausalLM(tf.LlamaConfig(
        hidden_size=lc.hidden, intermediate_size=lc.ffn, num_hidden_layers=lc.layers, num_attention_heads=lc.heads,
        num_key_value_heads=lc.kv_heads or lc.heads, vocab_size=lc.vocab, rms_norm_eps=lc.eps, max_position_embeddings=4096,
        rope_theta=lc.theta, bos_token_id=1, eos_token_id=2, pad_token_id=None, tie_word_embeddings=False)).eval()
    missing, unexpected = llm.load_state_dict({k: v for k, v in W["llama"].items()}, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    return llm


# ------------------------------------------------------------------------------------------------ against transformers, fp32
@pytest.mark.parametrize("kw", [{}, PROC], ids=["plain", "processors"])
def test_greedy_matches_transformers(dev, tiny, m32, embeds, hf_llm, kw):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    eos, pad = 53, m32.tokenizer.pad_token_id
    with torch.no_grad():
        hf = hf_llm.generate(inputs_embeds=embeds, attention_mask=torch.ones(embeds.shape[:2], dtype=torch.long), max_new_tokens=N_NEW,
                             do_sample=False, eos_token_id=eos, pad_token_id=pad, return_dict_in_generate=True, output_scores=True, **kw)
    want = hf_llm.compute_transition_scores(hf.sequences, hf.scores, normalize_logits=True)
    with with_eos(m32, eos), m32.llm_engine.adapters_disabled():
        out = scored(m32, audio, video, dev, **kw)
    assert out.sequences_scores is None and torch.equal(out.sequences, hf.sequences), (out.sequences, hf.sequences)
    n = lengths(out.sequences, eos)
    assert (n < out.sequences.shape[1]).any(), "a row should stop early, so that the masking is exercised"
    assert_masked(out, n)
    worst = worst_e = 0.0
    for r in range(out.sequences.shape[0]):
        worst = max(worst, float((out.token_scores[r, :n[r]] - want[r, :n[r]]).abs().max()))
        for j in range(int(n[r])):
            # entropy of the processed fp32 logits of this step, in float64
            p = torch.softmax(hf.scores[j][r].double(), -1)
            e = float(torch.special.entr(p).sum())
            worst_e = max(worst_e, abs(float(out.token_entropy[r, j]) - e))
            assert 0.0 <= float(out.token_entropy[r, j]) <= math.log(oc.llama.vocab)
    print(f"greedy {sorted(kw)}: max |token_scores - HF| {worst:.2e}, max |entropy - float64| {worst_e:.2e}")
    assert worst <= 1e-4 and worst_e <= 1e-4, (worst, worst_e)
    if kw:
        assert not (out.sequences == 7).any()


@pytest.mark.parametrize("eos", [53, 239])
def test_beam_n_best_matches_transformers(dev, tiny, m32, embeds, hf_llm, eos):  # noqa: F811
    """HF stores the processed log-probabilities (before the beam score is added) in `scores`, so compute_transition_scores with
    beam_indices and normalize_logits=False gives each token's own term of the beam score."""
    g, oc, W, audio, video, labels, prompt = tiny
    pad = m32.tokenizer.pad_token_id
    for kw in ({}, PROC):
        with torch.no_grad():
            hf = hf_llm.generate(inputs_embeds=embeds, attention_mask=torch.ones(embeds.shape[:2], dtype=torch.long), num_beams=4,
                                 num_return_sequences=3, max_new_tokens=N_NEW, do_sample=False, eos_token_id=eos, pad_token_id=pad,
                                 return_dict_in_generate=True, output_scores=True, **kw)
        want = hf_llm.compute_transition_scores(hf.sequences, hf.scores, hf.beam_indices, normalize_logits=False)
        with with_eos(m32, eos), m32.llm_engine.adapters_disabled():
            out = scored(m32, audio, video, dev, num_beams=4, num_return_sequences=3, **kw)
        assert torch.equal(out.sequences, hf.sequences), (eos, kw, out.sequences, hf.sequences)
        d_s = float((out.sequences_scores - hf.sequences_scores).abs().max())
        d_t = float((out.token_scores - want).abs().max())
        print(f"beam eos={eos} {sorted(kw)}: max |sequences_scores - HF| {d_s:.2e}, max |token_scores - HF| {d_t:.2e}")
        assert d_s < 1e-5 and d_t <= 1e-4, (eos, kw, d_s, d_t)


# ------------------------------------------------------------------------------------------------ the beam scorer's own sums
@pytest.mark.parametrize("kw", [{}, PROC], ids=["plain", "processors"])
@pytest.mark.parametrize("length_penalty", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_beam_token_scores_sum_to_the_sequence_score(dev, tiny, m32, m16, precision, nb, length_penalty, kw):  # noqa: F811
    """sum(token_scores) / len ** length_penalty is sequences_scores: the running beam score is a float32 sum of at most N of these very
    terms, so the two differ by at most N * ulp32(largest |partial sum|)."""
    g, oc, W, audio, video, labels, prompt = tiny
    m, eos = (m32 if precision == "fp32" else m16), 53
    with with_eos(m, eos):
        out = scored(m, audio, video, dev, num_beams=nb, num_return_sequences=nb, length_penalty=length_penalty, **kw)
        one = scored(m, audio, video, dev, num_beams=nb, length_penalty=length_penalty, **kw)
        ids, ids_s = gen(m, audio, video, dev, max_new_tokens=N_NEW, num_beams=nb, length_penalty=length_penalty, return_sequence_scores=True, **kw)
    B = audio.shape[0]
    assert out.sequences.shape[0] == B * nb == out.sequences_scores.shape[0] and out.token_scores.shape == out.sequences.shape
    n = lengths(out.sequences, eos)
    assert_masked(out, n)
    for r in range(B * nb):
        ts = out.token_scores[r, :n[r]].double()
        assert (ts <= 0).all() and torch.isfinite(ts).all()
        bound = N_NEW * float(np.spacing(np.float32(ts.cumsum(0).abs().max())))
        got = float(ts.sum()) / float(n[r]) ** length_penalty
        assert abs(got - float(out.sequences_scores[r])) <= bound, (precision, nb, length_penalty, r, got, float(out.sequences_scores[r]), bound)
        assert (out.token_entropy[r, :n[r]] >= 0).all() and (out.token_entropy[r, :n[r]] <= math.log(oc.llama.vocab)).all()
    # the n-best list: best first, distinct hypotheses, and its head is the 1-best call bit for bit
    L1 = one.sequences.shape[1]
    for b in range(B):
        rows = out.sequences[b * nb:(b + 1) * nb].tolist()
        assert len({tuple(r) for r in rows}) == nb, rows
        s = out.sequences_scores[b * nb:(b + 1) * nb]
        assert (s[:-1] >= s[1:]).all(), s
        for field in ("sequences", "token_scores", "token_entropy"):
            full, head = getattr(out, field)[b * nb], getattr(one, field)[b]
            assert torch.equal(full[:L1], head) and (full[L1:] == (m.tokenizer.pad_token_id if field == "sequences" else 0)).all(), (field, b)
        assert torch.equal(out.sequences_scores[b * nb].view(1).view(torch.int32), one.sequences_scores[b].view(1).view(torch.int32))
    # and without return_token_scores the call returns what it always did
    assert torch.equal(ids, one.sequences) and torch.equal(ids_s, one.sequences_scores)


# ------------------------------------------------------------------------------------------------ bf16
def token_logprobs_teacher_forced(m, x, ids, dev):
    """log_softmax of the model's own logits at every position of ids [B, L], one prefill per position (float64, CPU)."""
    eng = m.llm_engine
    B, S, _ = x.shape
    out = torch.zeros(ids.shape, dtype=torch.float64)
    xj = x
    for j in range(ids.shape[1]):
        if j:
            xj = torch.cat([x, ops.embedding(eng.embed, ids[:, :j].to(dev).contiguous())], 1)
        kc, vc = eng.alloc_cache(B, S + j)
        logits, _ = eng.prefill(xj.contiguous(), kc, vc)
        out[:, j] = torch.log_softmax(logits.float().cpu().double(), -1).gather(1, ids[:, j:j + 1])[:, 0]
    return out


def test_bf16_greedy_scores_are_teacher_forced(dev, tiny, m16):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    eos = 239
    with with_eos(m16, eos):
        out = scored(m16, audio, video, dev, max_new_tokens=6)
    with torch.no_grad():
        x = m16._llm_inputs(audio.to(dev), video.to(dev), None)
    want = token_logprobs_teacher_forced(m16, x, out.sequences, dev)
    n = lengths(out.sequences, eos)
    assert_masked(out, n)
    for r in range(out.sequences.shape[0]):
        d = (out.token_scores[r, :n[r]].double() - want[r, :n[r]]).abs().max()
        assert d <= 4 * BF16_LOGIT_MAX_ABS, (r, d, out.token_scores[r], want[r])


def test_fp4_weight_stream_scores(dev, tiny):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    m, eos = model16(tiny, "fp4"), 239
    with with_eos(m, eos):
        out = scored(m, audio, video, dev, max_new_tokens=6)
    assert out.token_scores.shape == out.sequences.shape == out.token_entropy.shape and out.token_scores.dtype == torch.float32
    assert torch.isfinite(out.token_scores).all() and (out.token_scores <= 0).all() and torch.isfinite(out.token_entropy).all()
    assert_masked(out, lengths(out.sequences, eos))


# ------------------------------------------------------------------------------------------------ sampling
def test_sampled_sequences_per_clip(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    kw = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, seed=5)
    with with_eos(m32, 53):
        out = scored(m32, audio, video, dev, num_return_sequences=3, **kw)
        rep = scored(m32, audio.repeat_interleave(3, 0), video.repeat_interleave(3, 0), dev, **kw)
        ids = gen(m32, audio, video, dev, max_new_tokens=N_NEW, num_return_sequences=3, **kw)
        greedy_like = scored(m32, audio, video, dev, do_sample=True, top_k=1, seed=5)
    assert out.sequences.shape[0] == 3 * audio.shape[0] and out.sequences_scores is None
    for a, b in zip(out, rep):
        assert a is b or torch.equal(a, b)
    assert torch.equal(ids, out.sequences)
    n = lengths(out.sequences, 53)
    assert_masked(out, n)
    p = torch.exp(out.token_scores)
    assert (p > 0).all() and (p <= 1).all()
    assert (out.token_scores[:, 0] < 0).all()                            # 40 candidates: no draw has probability one
    assert (out.token_entropy >= 0).all() and (out.token_entropy <= math.log(oc.llama.vocab)).all()    # of the untruncated distribution
    assert (greedy_like.token_scores == 0.0).all()


# ------------------------------------------------------------------------------------------------ defaults and errors
def test_defaults_return_what_they_did(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    ids = gen(m32, audio, video, dev, max_new_tokens=12)
    assert isinstance(ids, torch.Tensor) and torch.equal(ids, torch.from_numpy(np.asarray(g["generate_ids"])))
    out = scored(m32, audio, video, dev, max_new_tokens=12)
    assert torch.equal(out.sequences, ids)
    a = gen(m32, audio, video, dev, do_sample=True, seed=3)
    b = scored(m32, audio, video, dev, do_sample=True, seed=3)
    assert isinstance(a, torch.Tensor) and torch.equal(a, b.sequences)
    pair = gen(m32, audio, video, dev, num_beams=2, return_sequence_scores=True)
    assert isinstance(pair, tuple) and not isinstance(pair, GenerateOutput) and len(pair) == 2 and pair[1].shape == (audio.shape[0],)


def test_bad_arguments(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    for kw in ({"num_beams": 2, "num_return_sequences": 3}, {"num_return_sequences": 2}, {"num_return_sequences": 0},
               {"num_return_sequences": 1.5}, {"num_beams": 2, "num_return_sequences": 0}, {"return_sequence_scores": True}):
        with pytest.raises(ValueError):
            gen(m32, audio, video, dev, **kw)
    with pytest.raises(NotImplementedError):
        gen(m32, audio, video, dev, num_beams=2, do_sample=True)
