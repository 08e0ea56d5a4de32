"""ClipWhisperModel.generate(num_beams > 1) on the tiny golden model (tests/golden/g2_tiny_e2e.npz): beam search through the B*nb-row
token step, ops.beam_topk, HF's bookkeeping and ops.kv_gather_rows, against generate_ref.hf_beam_search, a CPU restatement of transformers'
GenerationMixin._beam_search (5.x, generation/utils.py) driving the oracle's llama_hidden with a KV cache that it reorders in full, as HF's
_reorder_cache does.  Where transformers is importable, the restatement and generate() are both pinned to LlamaForCausalLM.generate on the
same embeddings and weights.  Also: num_beams=1 is the golden greedy path, bf16 teacher-forced scores, fused / general token steps, row
independence and decode.py --num_beams."""
import functools
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import generate_ref  # noqa: E402
from avllm import ops  # noqa: E402
from bars import BF16_LOGIT_MAX_ABS  # noqa: E402
from generate_ref import hf_beam_search, oracle_step_fn, with_eos  # noqa: E402,F401
from oracle import avsr_oracle as O  # noqa: E402
from oracle import weights as Wt  # noqa: E402
from test_model_gpu import T, make_model, tiny  # noqa: E402,F401

N_NEW = 10
gen = functools.partial(generate_ref.gen, max_new_tokens=N_NEW)
# eos: tokens the tiny model's greedy decode emits at steps 2 and 1 (golden generate_ids rows [77 239 53 ...] and [151 77 239 ...]), so
# hypotheses finish early and length normalisation and padding are exercised
EOS_IDS = (53, 239)


@pytest.fixture(scope="module")
def m32(dev, tiny):  # noqa: F811
    g, oc, W, *_ = tiny
    return make_model(oc, W, "fp32", max_seq_len=256).eval()


@pytest.fixture(scope="module")
def embeds(dev, tiny):  # noqa: F811
    """The LLM inputs of the golden batch as the oracle computes them (CPU fp32), at the models' max_seq_len = 256."""
    g, oc, W, audio, video, labels, prompt = tiny
    oc256 = Wt.tiny()
    oc256.max_seq_len = 256
    with torch.no_grad():
        x, _ = O.encode(W, oc256, audio, video, None)
    return x


def test_one_beam_is_greedy(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    ids = gen(m32, audio, video, dev, max_new_tokens=12, num_beams=1)
    assert torch.equal(ids, T(g["generate_ids"]))


@pytest.mark.parametrize("eos", EOS_IDS)
@pytest.mark.parametrize("early_stopping", [False, True, "never"])
@pytest.mark.parametrize("length_penalty", [1.0, 0.0, 2.0])
@pytest.mark.parametrize("nb", [2, 4])
def test_fp32_matches_restatement(dev, tiny, m32, embeds, nb, length_penalty, early_stopping, eos):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    B, V, pad = embeds.shape[0], oc.llama.vocab, m32.tokenizer.pad_token_id
    want, want_s, _ = hf_beam_search(oracle_step_fn(W, oc, embeds, nb), B, nb, V, N_NEW, eos, pad, None, length_penalty, early_stopping)
    with with_eos(m32, eos):
        got, got_s = gen(m32, audio, video, dev, num_beams=nb, length_penalty=length_penalty, early_stopping=early_stopping,
                         return_sequence_scores=True)
    assert torch.equal(got, want), (got, want)
    assert (got_s - want_s).abs().max() < 1e-5, (got_s, want_s)
    if length_penalty == 1.0 and early_stopping is False:
        assert (got == eos).any(), "the case should finish hypotheses early"


def test_no_eos_runs_to_max_length(dev, tiny, m32, embeds):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    B, V, pad = embeds.shape[0], oc.llama.vocab, m32.tokenizer.pad_token_id
    want, want_s, _ = hf_beam_search(oracle_step_fn(W, oc, embeds, 3), B, 3, V, 7, None, pad)
    with with_eos(m32, None):
        got, got_s = gen(m32, audio, video, dev, num_beams=3, max_new_tokens=7, return_sequence_scores=True)
    assert got.shape == (B, 7) and torch.equal(got, want)
    assert (got_s - want_s).abs().max() < 1e-5


def test_pinned_to_transformers(dev, tiny, m32, embeds):  # noqa: F811
    """LlamaForCausalLM.generate(inputs_embeds=..., num_beams=...) on the golden LLM weights (adapters off on both sides): its sequences and
    sequences_scores equal the restatement's and generate()'s."""
    tf = pytest.importorskip("transformers")
    g, oc, W, audio, video, labels, prompt = tiny
    lc = oc.llama
    llm = tf.LlamaForCausalLM(tf.LlamaConfig(
        hidden_size=lc.hidden, intermediate_size=lc.ffn, num_hidden_layers=lc.layers, num_attention_heads=lc.heads,
        num_key_value_heads=lc.kv_heads or lc.heads, vocab_size=lc.vocab, rms_norm_eps=lc.eps, max_position_embeddings=4096,
        rope_theta=lc.theta, bos_token_id=1, eos_token_id=2, pad_token_id=None, tie_word_embeddings=False)).eval()
    missing, unexpected = llm.load_state_dict({k: v for k, v in W["llama"].items()}, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    B, V, pad = embeds.shape[0], lc.vocab, m32.tokenizer.pad_token_id
    for nb, lp, es, eos in ((4, 1.0, False, 53), (2, 2.0, True, 239), (4, 0.0, "never", 239)):
        with torch.no_grad():
            hf = llm.generate(inputs_embeds=embeds, attention_mask=torch.ones(embeds.shape[:2], dtype=torch.long), num_beams=nb,
                              max_new_tokens=N_NEW, do_sample=False, length_penalty=lp, early_stopping=es, eos_token_id=eos,
                              pad_token_id=pad, return_dict_in_generate=True, output_scores=True, num_return_sequences=1)
        want, want_s, _ = hf_beam_search(oracle_step_fn(W, oc, embeds, nb, lora=False), B, nb, V, N_NEW, eos, pad, None, lp, es)
        assert torch.equal(hf.sequences, want), (nb, lp, es, hf.sequences, want)
        assert (hf.sequences_scores - want_s).abs().max() < 1e-5
        with with_eos(m32, eos), m32.llm_engine.adapters_disabled():
            got, got_s = gen(m32, audio, video, dev, num_beams=nb, length_penalty=lp, early_stopping=es, return_sequence_scores=True)
        assert torch.equal(got, hf.sequences), (nb, lp, es, got, hf.sequences)
        assert (got_s - hf.sequences_scores).abs().max() < 1e-5


def seq_logprob(m, x, ids, pad, eos, dev):
    """Sum of the model's own log-probabilities along each hypothesis (prefill over the prompt plus the tokens before each position),
    stopping after its first eos; and its length."""
    eng = m.llm_engine
    B, S, _ = x.shape
    tot, lens = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.int64)
    xj = x
    for j in range(ids.shape[1]):
        if j:
            xj = torch.cat([x, ops.embedding(eng.embed, ids[:, :j].to(dev).contiguous())], 1)
        kc, vc = eng.alloc_cache(B, S + j)
        logits, _ = eng.prefill(xj.contiguous(), kc, vc)
        lp = torch.log_softmax(logits.float().cpu(), -1).double()
        for b in range(B):
            if j == 0 or (lens[b] == j and int(ids[b, j - 1]) != eos):
                tot[b] += lp[b, int(ids[b, j])]
                lens[b] = j + 1
    return tot, lens


def test_bf16_scores_are_teacher_forced_and_beat_greedy(dev, tiny):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    m = make_model(oc, W, "bf16", max_seq_len=256).eval()
    eos, pad = 53, m.tokenizer.pad_token_id
    with with_eos(m, eos):
        ids, scores = gen(m, audio, video, dev, num_beams=4, return_sequence_scores=True)
        greedy = gen(m, audio, video, dev)
    with torch.no_grad():
        x = m._llm_inputs(audio.to(dev), video.to(dev), None)
    tot, lens = seq_logprob(m, x, ids, pad, eos, dev)
    tol = 4 * BF16_LOGIT_MAX_ABS * lens.double()            # each step's log-probability within twice the logit bar, both paths
    assert ((scores.double() - tot / lens.double()).abs() <= tol / lens.double()).all(), (scores, tot / lens)
    gt, gl = seq_logprob(m, x, greedy, pad, eos, dev)
    assert (scores.double() >= gt / gl.double() - tol / lens.double()).all(), (scores, gt / gl)


@pytest.mark.parametrize("B,nb,fused", [(4, 4, True), (8, 4, False)])
def test_bf16_fused_and_general_token_step(dev, tiny, B, nb, fused):  # noqa: F811
    """B*nb = 16 rows take the fused bf16 step, 32 the general one; both give teacher-forced scores."""
    g, oc, W, audio, video, labels, prompt = tiny
    m = make_model(oc, W, "bf16", max_seq_len=256).eval()
    assert m.llm_engine.decode_is_fused(B * nb) == fused
    rep = lambda t: t.repeat((B + 1) // 2, *([1] * (t.dim() - 1)))[:B]  # noqa: E731
    a, v = rep(audio) * torch.linspace(0.5, 1.5, B).view(B, *([1] * (audio.dim() - 1))), rep(video)
    with with_eos(m, 239):
        ids, scores = gen(m, a, v, dev, num_beams=nb, max_new_tokens=6, return_sequence_scores=True)
    with torch.no_grad():
        x = m._llm_inputs(a.to(dev), v.to(dev), None)
    tot, lens = seq_logprob(m, x, ids, m.tokenizer.pad_token_id, 239, dev)
    assert ((scores.double() - tot / lens.double()).abs() <= 4 * BF16_LOGIT_MAX_ABS).all(), (scores, tot / lens)


def test_rows_are_independent(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    with with_eos(m32, 53):
        both, s_both = gen(m32, audio, video, dev, num_beams=4, return_sequence_scores=True)
        for b in range(audio.shape[0]):
            one, s_one = gen(m32, audio[b:b + 1], video[b:b + 1], dev, num_beams=4, return_sequence_scores=True)
            n = one.shape[1]
            assert torch.equal(both[b, :n], one[0]) and (both[b, n:] == m32.tokenizer.pad_token_id).all()
            assert abs(float(s_both[b]) - float(s_one[0])) < 1e-5


def test_bad_arguments(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    with pytest.raises(NotImplementedError):
        gen(m32, audio, video, dev, num_beams=2, do_sample=True)
    for kw in ({"num_beams": 0}, {"num_beams": 17}, {"num_beams": 2, "early_stopping": "sometimes"}, {"return_sequence_scores": True}):
        with pytest.raises(ValueError):
            gen(m32, audio, video, dev, **kw)


def test_decode_script_beams(dev, tmp_path):
    """decode.py --num_beams 4 twice: identical results; without --num_beams the output is the greedy one (--num_beams 1)."""
    from test_data_cpu import make_set
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = tmp_path / "toy"
    data.mkdir()
    mp, lp = make_set(data, n=4)
    env = dict(os.environ, PYTHONPATH=root)

    def run(name, *extra):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(root, "scripts/clip_whisper/decode.py"), "--test_data", str(mp), "--test_wrd", str(lp),
                            "--output_dir", str(out), "--batch_size", "2", "--max_new_tokens", "6", "--tiny", "--data_path", str(data), *extra],
                           capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return [x["hypothesis"] for x in json.load(open(glob.glob(str(out / "decode_results.json"))[0]))["results"]]

    b1 = run("b1", "--num_beams", "4", "--length_penalty", "1.0")
    b2 = run("b2", "--num_beams", "4", "--length_penalty", "1.0")
    assert b1 == b2 and len(b1) == 4
    assert run("g") == run("g1", "--num_beams", "1")
