"""ClipWhisperModel.generate(repetition_penalty=..., no_repeat_ngram_size=..., min_new_tokens=...) on the tiny golden model
(tests/golden/g2_tiny_e2e.npz), greedy, sampled and beam search.

fp32: tokens identical to a restatement loop on the CPU: the oracle's logits -> test_logits_process_cpu.restate (HF's three processors) ->
the selection (argmax; the sampling chain of test_sample_gpu.kept plus generate_ref.draw, the kernel's inverse-CDF draw;
generate_ref.hf_beam_search with the processors between the log_softmax and the beam scores, as
GenerationMixin._beam_search has them), and where transformers imports to LlamaForCausalLM.generate with the same keywords.
The cases were chosen on the CPU so that the restatement's decisions are clear of the fp32 logit bar (tests/bars.py F32_LOGITS_ABS = 1e-3
on each logit, so 2e-3 on a difference) at every step; each test asserts that margin again, no case is dropped at run time:
  greedy   top-1 minus top-2 of the processed logits > 2e-3 (checked: the grids GREEDY_CASES were picked from, eos in {None, 53, 239},
           p in {1.0, 1.2, 1.3, 2.0}, n in {0, 2, 3}, m in {0, 6, 8}, 12 new tokens);
  sampled  temperature 0.1, filters off: the uniform draw u lies more than 2e-3 / 0.1 = 2e-2 inside its token's CDF interval (a logit
           error e moves a scaled logit by e / t and every cumulative probability by less than that; seeds 0..399 were searched);
  beams    at every step the three selections (the 2*nb best candidates, the nb running beams among them, the nb finished hypotheses)
           have more than 2e-3 between the last score taken and the first one left out; the order inside a selected set only permutes
           the beams.
Each case also shows that the knob did something: the unprocessed output repeats an n-gram (or ends before min_new_tokens) and the processed
one does not.

bf16 (fused and general token step, bf16 and fp8 weight streams): properties only."""
import contextlib
import functools
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import generate_ref  # noqa: E402
from avllm import ops  # noqa: E402
from bars import F32_LOGITS_ABS  # noqa: E402
from generate_ref import hf_beam_search, oracle_step_fn, token_loop, trim, with_eos  # noqa: E402
from test_generate_beam_gpu import embeds  # noqa: E402,F401
from test_generate_sample_gpu import BOUNDARY_TOL  # noqa: E402
from test_logits_process_cpu import restate  # noqa: E402
from test_model_gpu import make_model, tiny  # noqa: E402,F401
from test_sample_gpu import kept  # noqa: E402

N_NEW = 12
gen = functools.partial(generate_ref.gen, max_new_tokens=N_NEW)
MARGIN = 2 * F32_LOGITS_ABS
# (eos, repetition_penalty, no_repeat_ngram_size, min_new_tokens, n-gram size the unprocessed output repeats and the processed must not (0:
# none), the unprocessed output ends before min_new_tokens, adapters on: with them the penalised cases have a 8e-4 margin at one step)
GREEDY_CASES = [
    (None, 1.0, 2, 0, 2, False, True),
    (None, 1.0, 3, 0, 3, False, True),
    (53, 1.0, 3, 8, 3, True, True),
    (239, 1.0, 0, 6, 0, True, True),
    (None, 1.3, 0, 0, 2, False, False),
    (None, 1.2, 3, 0, 3, False, False),
    (53, 1.2, 2, 6, 2, True, False),
]
SAMPLE_T = 0.1
# (seed, eos, repetition_penalty, no_repeat_ngram_size, min_new_tokens, n-gram size repeated without the knobs, early end without them)
SAMPLE_CASES = [
    (97, None, 1.3, 2, 0, 2, False),
    (221, None, 1.0, 2, 0, 2, False),
    (13, 239, 1.3, 2, 6, 0, True),
]
# (num_beams, eos, repetition_penalty, no_repeat_ngram_size, min_new_tokens, length_penalty, early_stopping, n-gram size repeated without
# the knobs, early end without them); the grid nb in {2, 4}, eos in {None, 53, 239}, p in {1.0, 1.3}, n in {0, 2, 3}, m in {0, 6} was
# searched: the penalised beam cases all have an edge gap under 2e-3 at some step (the log-probability mode is pinned bit for bit in
# tests/test_logits_process_gpu.py, and by properties below)
BEAM_CASES = [
    (2, 53, 1.0, 0, 6, 1.0, False, 0, True),
    (2, 53, 1.0, 2, 6, 1.0, False, 2, True),
]


def processors(p, n, m, eos):
    """HF's three processors as generate_ref's process(scores, hist)."""
    return lambda s, hist: restate(s, hist, p, n, m, eos)


def has_repeat(row, n):
    """True when an n-gram occurs twice in the token list."""
    grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1)]
    return len(set(grams)) < len(grams)


@pytest.fixture(scope="module")
def m32(dev, tiny):  # noqa: F811
    g, oc, W, *_ = tiny
    return make_model(oc, W, "fp32", max_seq_len=256).eval()


def knob_did_something(plain, got, eos, pad, n_rep, m, early):
    """The unprocessed output shows the failure the knob is for, the processed one does not."""
    plain, got = [trim(r, eos, pad) for r in plain], [trim(r, eos, pad) for r in got]
    if n_rep:
        assert any(has_repeat(r, n_rep) for r in plain), plain
        assert not any(has_repeat(r, n_rep) for r in got), got
    if early:
        assert any(eos in r[:m] for r in plain), plain
        assert not any(eos in r[:m] for r in got), got


@pytest.mark.parametrize("eos,p,n,m,n_rep,early,lora", GREEDY_CASES)
def test_greedy_fp32_matches_restatement(dev, tiny, m32, embeds, eos, p, n, m, n_rep, early, lora):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    B, pad = embeds.shape[0], m32.tokenizer.pad_token_id
    want, margin = token_loop(oracle_step_fn(W, oc, embeds, 1, lora=lora), B, N_NEW, eos, pad, processors(p, n, m, eos))
    print(f"greedy eos={eos} p={p} n={n} m={m}: smallest top-2 margin {margin:.3e}")
    assert margin > MARGIN, margin
    plain, _ = token_loop(oracle_step_fn(W, oc, embeds, 1, lora=lora), B, N_NEW, eos, pad, processors(1.0, 0, 0, eos))
    knob_did_something(plain.tolist(), want.tolist(), eos, pad, n_rep, m, early)
    with with_eos(m32, eos), (contextlib.nullcontext() if lora else m32.llm_engine.adapters_disabled()):
        got = gen(m32, audio, video, dev, repetition_penalty=p, no_repeat_ngram_size=n, min_new_tokens=m)
        assert torch.equal(gen(m32, audio, video, dev), plain)
    assert torch.equal(got, want), (got, want)


@pytest.mark.parametrize("seed,eos,p,n,m,n_rep,early", SAMPLE_CASES)
def test_sampled_fp32_matches_restatement(dev, tiny, m32, embeds, seed, eos, p, n, m, n_rep, early):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    B, pad = embeds.shape[0], m32.tokenizer.pad_token_id
    want, margin = token_loop(oracle_step_fn(W, oc, embeds, 1), B, N_NEW, eos, pad, processors(p, n, m, eos), sample=(SAMPLE_T, 0, 1.0, seed))
    print(f"sampled seed={seed} eos={eos} p={p} n={n} m={m}: smallest CDF margin {margin:.3e}")
    assert margin > MARGIN / SAMPLE_T, margin
    plain, _ = token_loop(oracle_step_fn(W, oc, embeds, 1), B, N_NEW, eos, pad, processors(1.0, 0, 0, eos), sample=(SAMPLE_T, 0, 1.0, seed))
    knob_did_something(plain.tolist(), want.tolist(), eos, pad, n_rep, m, early)
    with with_eos(m32, eos):
        got = gen(m32, audio, video, dev, do_sample=True, temperature=SAMPLE_T, top_k=0, top_p=1.0, seed=seed, repetition_penalty=p,
                  no_repeat_ngram_size=n, min_new_tokens=m)
    assert torch.equal(got, want), (got, want)


@pytest.mark.parametrize("nb,eos,p,n,m,lp,es,n_rep,early", BEAM_CASES)
def test_beam_fp32_matches_restatement(dev, tiny, m32, embeds, nb, eos, p, n, m, lp, es, n_rep, early):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    B, V, pad = embeds.shape[0], oc.llama.vocab, m32.tokenizer.pad_token_id
    want, want_s, gap = hf_beam_search(oracle_step_fn(W, oc, embeds, nb), B, nb, V, N_NEW, eos, pad, processors(p, n, m, eos), lp, es)
    print(f"beams nb={nb} eos={eos} p={p} n={n} m={m}: smallest candidate gap {gap:.3e}")
    assert gap > MARGIN, gap
    plain, _, _ = hf_beam_search(oracle_step_fn(W, oc, embeds, nb), B, nb, V, N_NEW, eos, pad, processors(1.0, 0, 0, eos), lp, es)
    knob_did_something(plain.tolist(), want.tolist(), eos, pad, n_rep, m, early)
    with with_eos(m32, eos):
        got, got_s = gen(m32, audio, video, dev, num_beams=nb, length_penalty=lp, early_stopping=es, return_sequence_scores=True,
                         repetition_penalty=p, no_repeat_ngram_size=n, min_new_tokens=m)
    assert torch.equal(got, want), (got, want)
    assert (got_s - want_s).abs().max() < 1e-5, (got_s, want_s)


def test_pinned_to_transformers(dev, tiny, m32, embeds):  # noqa: F811
    """LlamaForCausalLM.generate(inputs_embeds=..., repetition_penalty=..., no_repeat_ngram_size=..., min_new_tokens=...) on the golden LLM
    weights (adapters off on both sides), greedy and beam search: its sequences equal the restatement's and generate()'s."""
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
    mask = torch.ones(embeds.shape[:2], dtype=torch.long)
    for nb, eos, p, n, m in PINNED_CASES:
        kw = dict(repetition_penalty=p, no_repeat_ngram_size=n, min_new_tokens=m)
        with torch.no_grad():
            hf = llm.generate(inputs_embeds=embeds, attention_mask=mask, num_beams=nb, max_new_tokens=N_NEW, do_sample=False, eos_token_id=eos,
                              pad_token_id=pad, return_dict_in_generate=True, output_scores=True, num_return_sequences=1, **kw)
        if nb == 1:
            want, margin = token_loop(oracle_step_fn(W, oc, embeds, 1, lora=False), B, N_NEW, eos, pad, processors(p, n, m, eos))
        else:
            want, want_s, margin = hf_beam_search(oracle_step_fn(W, oc, embeds, nb, lora=False), B, nb, V, N_NEW, eos, pad, processors(p, n, m, eos))
            assert (hf.sequences_scores - want_s).abs().max() < 1e-5
        assert margin > MARGIN, (nb, eos, p, n, m, margin)
        assert torch.equal(hf.sequences, want), (nb, eos, p, n, m, hf.sequences, want)
        with with_eos(m32, eos), m32.llm_engine.adapters_disabled():
            got = gen(m32, audio, video, dev, num_beams=nb, **kw)
        assert torch.equal(got, hf.sequences), (nb, eos, p, n, m, got, hf.sequences)


# (num_beams, eos, repetition_penalty, no_repeat_ngram_size, min_new_tokens), adapters off
PINNED_CASES = [
    (1, 53, 1.2, 2, 6),
    (1, 53, 1.0, 3, 8),
    (2, 53, 1.0, 0, 6),
]


# ------------------------------------------------------------------------------------------------ bf16 properties
def model16(tiny, decode_weights):  # noqa: F811
    """The bf16 tiny model, adapters off (the fp8 weight stream covers the frozen projections), with bf16 or fp8 token-step weights."""
    from avllm.arch import ClipCfg, LlamaCfg, LoraCfg, ModelCfg, WhisperCfg
    from avllm.model import ClipWhisperModel
    g, oc, W, *_ = tiny
    cfg = ModelCfg(WhisperCfg(**vars(oc.whisper)), ClipCfg(**vars(oc.clip)), LlamaCfg(**vars(oc.llama)), LoraCfg(oc.lora.r, oc.lora.alpha))
    return ClipWhisperModel(device="cuda:0", use_lora=False, lora_r=oc.lora.r, lora_alpha=oc.lora.alpha, lora_dropout=0.0, max_seq_len=256,
                            config=cfg, weights={k: v for k, v in W.items() if k != "lora"}, precision="bf16",
                            decode_weights=decode_weights).eval()


def batch(tiny, B):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    rep = lambda t: t.repeat((B + 1) // 2, *([1] * (t.dim() - 1)))[:B]  # noqa: E731
    return rep(audio) * torch.linspace(0.5, 1.5, B).view(B, *([1] * (audio.dim() - 1))), rep(video)


MODES = {"greedy": {}, "sampled": dict(do_sample=True, temperature=1.0, top_k=20, top_p=0.9, seed=3), "beams": dict(num_beams=4)}


@pytest.mark.parametrize("decode_weights", ["bf16", "fp8"])
@pytest.mark.parametrize("B,fused", [(2, True), (20, False)])
@pytest.mark.parametrize("mode", list(MODES))
def test_bf16_properties(dev, tiny, mode, B, fused, decode_weights):  # noqa: F811
    """No n-gram of size n twice in a returned row, no EOS before min_new_tokens, rows independent of their batch neighbours, and the three
    defaults passed explicitly change nothing."""
    m = model16(tiny, decode_weights)
    a, v = batch(tiny, B)
    rows = B * (4 if mode == "beams" else 1)
    assert m.llm_engine.decode_is_fused(rows) == fused
    assert m.llm_engine.decode_streams_fp8(rows) == (fused and decode_weights == "fp8")
    eos, pad, n, mn = 239, m.tokenizer.pad_token_id, 2, 6
    kw = dict(MODES[mode], max_new_tokens=16)
    with with_eos(m, eos):
        plain = gen(m, a, v, dev, **kw)
        assert torch.equal(gen(m, a, v, dev, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, **kw), plain)
        got = gen(m, a, v, dev, repetition_penalty=1.3, no_repeat_ngram_size=n, min_new_tokens=mn, **kw)
        for r in got.tolist():
            r = trim(r, eos, pad)
            assert not has_repeat(r, n), r
            assert eos not in r[:mn] and len(r) >= mn, r
        if mode != "sampled":                               # a sampled row's seed is seed + its batch index
            # the same rows in reverse order: other neighbours and positions, the same token-step path (a batch of another size may take the
            # other bf16 path, whose rounding differs)
            back = gen(m, a.flip(0), v.flip(0), dev, repetition_penalty=1.3, no_repeat_ngram_size=n, min_new_tokens=mn, **kw)
            assert torch.equal(back.flip(0), got), (back.flip(0), got)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sampled_tokens_lie_in_the_kept_set_of_the_processed_logits(dev, tiny, precision):  # noqa: F811
    """test_generate_sample_gpu's teacher-forced membership test on the processed logits: each drawn token is in the kept set of
    restate(eval-forward logits of the prompt plus the tokens before it, those tokens)."""
    g, oc, W, audio, video, labels, prompt = tiny
    m = make_model(oc, W, precision, max_seq_len=256).eval()
    m.eos_token_id = None
    t, k, tp, p, n = 1.0, 50, 0.9, 1.3, 2
    ids = gen(m, audio, video, dev, do_sample=True, temperature=t, top_k=k, top_p=tp, seed=11, repetition_penalty=p, no_repeat_ngram_size=n)
    eng = m.llm_engine
    with torch.no_grad():
        x = m._llm_inputs(audio.to(dev), video.to(dev), None)
    B, S, _ = x.shape
    checked = 0
    for j in range(ids.shape[1]):
        xj = torch.cat([x, ops.embedding(eng.embed, ids[:, :j].to(dev).contiguous())], 1) if j else x
        kc, vc = eng.alloc_cache(B, S + j)
        logits, _ = eng.prefill(xj, kc, vc)
        lf = restate(logits.float().cpu(), ids[:, :j], p, n, 0, None).numpy()
        for b in range(B):
            keep, _ = kept(lf[b], t, k, tp)
            xs = lf[b] / np.float32(t)
            margin = xs[keep].min() - (xs[~keep].max() if (~keep).any() else -np.inf)
            tok = int(ids[b, j])
            assert np.isfinite(xs[tok]), (precision, j, b, tok)          # a banned token has mass 0
            if margin >= BOUNDARY_TOL[precision]:
                assert keep[tok], (precision, j, b, tok)
                checked += 1
            else:
                assert xs[tok] >= xs[keep].min() - 2 * BOUNDARY_TOL[precision], (precision, j, b, tok, xs[tok], xs[keep].min())
    assert precision != "fp32" or checked >= ids.numel() // 2, checked
    assert not any(has_repeat(r, n) for r in ids.tolist())


def test_bad_arguments_raise_before_any_gpu_work(dev, tiny, m32, monkeypatch):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny

    def no_gpu_work(*a, **k):
        raise AssertionError("the arguments must be refused before the encoders run")
    monkeypatch.setattr(m32, "_llm_inputs", no_gpu_work)
    for kw in ({"repetition_penalty": 0}, {"repetition_penalty": -1}, {"repetition_penalty": "x"}, {"no_repeat_ngram_size": -1},
               {"no_repeat_ngram_size": 1.5}, {"min_new_tokens": -1}, {"repetition_penalty": 1.2, "max_new_tokens": 1025}):
        for mode in MODES.values():
            with pytest.raises(ValueError):
                gen(m32, audio, video, dev, **dict(mode, **kw))


def test_decode_script_processors(dev, tmp_path):
    """decode.py with the three flags: runs, repeats itself, differs from the plain run and equals it when the flags carry the defaults."""
    from test_data_cpu import make_set
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = tmp_path / "toy"
    data.mkdir()
    mp, lp = make_set(data, n=4)
    env = dict(os.environ, PYTHONPATH=root)

    def run(name, *extra):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(root, "scripts/clip_whisper/decode.py"), "--test_data", str(mp), "--test_wrd", str(lp),
                            "--output_dir", str(out), "--batch_size", "2", "--max_new_tokens", "8", "--tiny", "--data_path", str(data), *extra],
                           capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return [x["hypothesis"] for x in json.load(open(glob.glob(str(out / "decode_results.json"))[0]))["results"]]

    flags = ("--repetition_penalty", "1.3", "--no_repeat_ngram_size", "2", "--min_new_tokens", "4")
    p1, p2 = run("p1", *flags), run("p2", *flags)
    assert p1 == p2 and len(p1) == 4
    plain = run("g")
    assert plain == run("d", "--repetition_penalty", "1.0", "--no_repeat_ngram_size", "0", "--min_new_tokens", "0")
    assert p1 != plain
    assert len(run("b", "--num_beams", "2", *flags)) == 4
