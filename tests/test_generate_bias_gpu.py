"""ClipWhisperModel.generate(sequence_bias=..., bad_words_ids=..., suppress_tokens=..., begin_suppress_tokens=..., hotwords=...) on the tiny
golden model (tests/golden/g2_tiny_e2e.npz), greedy, sampled and beam search.

fp32: tokens identical to a restatement loop on the CPU: the oracle's logits -> logits_bias_ref.chain (HF's seven processors, held to
transformers' classes in tests/test_logits_bias_cpu.py) -> the selection (argmax; the sampling chain of test_sample_gpu.kept with the
kernel's inverse-CDF draw; HF's beam search with the processors between the log_softmax and the beam scores), and where transformers
imports to LlamaForCausalLM.generate with the same keywords.  The cases were chosen on the CPU so that every decision of the restatement
is clear of the fp32 logit bar (tests/bars.py F32_LOGITS_ABS = 1e-3 on each logit, so 2e-3 on a difference), exactly as
tests/test_generate_processors_gpu.py states it for its cases; each test asserts that margin again and no case is dropped at run time.
Each case also shows that its knob acted (see `acted`).

bf16 (fused and general token step; bf16, fp8 and fp4 weight streams): properties only."""
import contextlib
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
from avllm.model import hotword_sequence_bias  # noqa: E402
from bars import F32_LOGITS_ABS  # noqa: E402
from generate_ref import hf_beam_search, oracle_step_fn, token_loop, trim, with_eos  # noqa: E402
from logits_bias_ref import chain  # noqa: E402
from test_generate_beam_gpu import embeds  # noqa: E402,F401
from test_generate_processors_gpu import batch  # noqa: E402
from test_model_gpu import make_model, tiny  # noqa: E402,F401

N_NEW = 12
gen = functools.partial(generate_ref.gen, max_new_tokens=N_NEW)
MARGIN = 2 * F32_LOGITS_ABS
SAMPLE_T = 0.1
OFF = dict(sequence_bias=None, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None)

# Each case: (eos, the keywords, what shows that they acted).  The checks of `acted`, on the rows without their padding:
#   ("gone", [tokens])         the token sequence occurs in the output without the keywords and not with them
#   ("new", [tokens])          it occurs with them and not without
#   ("moved", token)           the token is at position 0 of a row without them, at position 0 of no row with them, and later in a row
# Searched on the CPU: eos in {None, 53, 239} (beams: also 83, 124, 37, 151), every token, bigram and first token of the unprocessed output
# as the thing to suppress or ban, every 1- and 2-token prefix of it followed by one of {9, 100, 201} as the sequence to boost with 12.0 or
# 25.0, sampling seeds 0..119; the smallest margins of the chosen cases: greedy 1.4e-2, sampled 6.4e-3 * 10, beams 3.5e-3.
GREEDY_CASES = [
    (None, dict(suppress_tokens=[53], sequence_bias={(239, 201): 12.0}), [("gone", [53]), ("new", [239, 201])]),
    (53, dict(bad_words_ids=[[239, 77]], sequence_bias={(77, 239, 9): 12.0}), [("gone", [239, 77]), ("new", [77, 239, 9])]),
    (None, dict(bad_words_ids=[[239, 53], [53]], begin_suppress_tokens=[77, 151]), [("gone", [239, 53]), ("gone", [53]), ("moved", 77)]),
    (239, dict(begin_suppress_tokens=[77], suppress_tokens=[151]), [("moved", 77), ("gone", [151])]),
    (None, dict(hotwords=["yP", "J2"], hotword_bias=5.0), [("new", [124, 83])]),            # "yP" is the byte tokens 124, 83
]
SAMPLE_CASES = [           # (seed, eos, keywords, checks)
    (112, 239, dict(suppress_tokens=[151], sequence_bias={(77, 201): 12.0}), [("gone", [151]), ("new", [77, 201])]),
    (36, 239, dict(begin_suppress_tokens=[77]), [("moved", 77)]),
    (44, 53, dict(bad_words_ids=[[239, 77]]), [("gone", [239, 77])]),
    (81, 53, dict(sequence_bias={(77, 239, 9): 12.0}), [("new", [77, 239, 9])]),
]
BEAM_CASES = [             # (num_beams, eos, keywords, checks, adapters on)
    (2, 151, dict(sequence_bias={(239, 201): 12.0}, begin_suppress_tokens=[77]), [("new", [239, 201]), ("moved", 77)], True),
    (2, 239, dict(suppress_tokens=[83]), [("gone", [83])], True),
    (2, 239, dict(bad_words_ids=[[83]]), [("gone", [83])], True),
    (2, 83, dict(sequence_bias={(77, 239, 201): 12.0}), [("new", [77, 239, 201])], True),
    (2, 151, dict(bad_words_ids=[[239, 53]]), [("gone", [239, 53])], False),
]
PINNED_CASES = [           # (num_beams, eos, keywords), adapters off
    (1, None, dict(suppress_tokens=[53], sequence_bias={(239, 201): 12.0})),
    (1, 53, dict(bad_words_ids=[[239, 77]], begin_suppress_tokens=[77])),
    (2, 151, dict(bad_words_ids=[[239, 53]])),
    (2, 151, dict(begin_suppress_tokens=[77])),
    (2, 151, dict(sequence_bias={(83, 201): 12.0})),
]


def process_fn(eos, kw):
    return lambda s, hist: chain(s, hist, eos=eos, **kw)


def occurs(rows, seq):
    seq = list(seq)
    return any(r[i:i + len(seq)] == seq for r in rows for i in range(len(r) - len(seq) + 1))


def acted(plain, got, eos, pad, checks):
    """The output without the keywords shows what each is for, the output with them does not (or the reverse for a boosted sequence)."""
    plain, got = [trim(r, eos, pad) for r in plain], [trim(r, eos, pad) for r in got]
    assert checks
    for kind, what in checks:
        if kind == "gone":
            assert occurs(plain, what) and not occurs(got, what), (kind, what, plain, got)
        elif kind == "new":
            assert occurs(got, what) and not occurs(plain, what), (kind, what, plain, got)
        elif kind == "moved":
            assert any(r[0] == what for r in plain) and not any(r[0] == what for r in got) and any(what in r[1:] for r in got), \
                (kind, what, plain, got)
        else:
            raise AssertionError(kind)


def full(kw, tokenizer=None):
    """The chain's keywords for generate()'s: hotwords become the sequence_bias entries generate() makes of them."""
    kw = dict(OFF, **kw)
    if "hotwords" in kw:
        kw["sequence_bias"] = hotword_sequence_bias(tokenizer, kw.pop("hotwords"), kw.pop("hotword_bias"), kw["sequence_bias"])
    return kw


@pytest.fixture(scope="module")
def m32(dev, tiny):  # noqa: F811
    g, oc, W, *_ = tiny
    return make_model(oc, W, "fp32", max_seq_len=256).eval()


def adapters(m, lora):
    return contextlib.nullcontext() if lora else m.llm_engine.adapters_disabled()


@pytest.mark.parametrize("eos,kw,checks", GREEDY_CASES)
def test_greedy_fp32_matches_restatement(dev, tiny, m32, embeds, eos, kw, checks):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    B, pad = embeds.shape[0], m32.tokenizer.pad_token_id
    want, margin = token_loop(oracle_step_fn(W, oc, embeds, 1), B, N_NEW, eos, pad, process_fn(eos, full(kw, m32.tokenizer)))
    print(f"greedy eos={eos} {kw}: smallest top-2 margin {margin:.3e}")
    assert margin > MARGIN, margin
    plain, _ = token_loop(oracle_step_fn(W, oc, embeds, 1), B, N_NEW, eos, pad, process_fn(eos, OFF))
    acted(plain.tolist(), want.tolist(), eos, pad, checks)
    with with_eos(m32, eos):
        got = gen(m32, audio, video, dev, **kw)
    assert torch.equal(got, want), (got, want)


@pytest.mark.parametrize("seed,eos,kw,checks", SAMPLE_CASES)
def test_sampled_fp32_matches_restatement(dev, tiny, m32, embeds, seed, eos, kw, checks):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    B, pad = embeds.shape[0], m32.tokenizer.pad_token_id
    sample = (SAMPLE_T, 0, 1.0, seed)
    want, margin = token_loop(oracle_step_fn(W, oc, embeds, 1), B, N_NEW, eos, pad, process_fn(eos, full(kw)), sample=sample)
    print(f"sampled seed={seed} eos={eos} {kw}: smallest CDF margin {margin:.3e}")
    assert margin > MARGIN / SAMPLE_T, margin
    plain, _ = token_loop(oracle_step_fn(W, oc, embeds, 1), B, N_NEW, eos, pad, process_fn(eos, OFF), sample=sample)
    acted(plain.tolist(), want.tolist(), eos, pad, checks)
    with with_eos(m32, eos):
        got = gen(m32, audio, video, dev, do_sample=True, temperature=SAMPLE_T, top_k=0, top_p=1.0, seed=seed, **kw)
    assert torch.equal(got, want), (got, want)


@pytest.mark.parametrize("nb,eos,kw,checks,lora", BEAM_CASES)
def test_beam_fp32_matches_restatement(dev, tiny, m32, embeds, nb, eos, kw, checks, lora):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    B, V, pad = embeds.shape[0], oc.llama.vocab, m32.tokenizer.pad_token_id
    want, want_s, gap = hf_beam_search(oracle_step_fn(W, oc, embeds, nb, lora=lora), B, nb, V, N_NEW, eos, pad, process_fn(eos, full(kw)))
    print(f"beams nb={nb} eos={eos} {kw}: smallest candidate gap {gap:.3e}")
    assert gap > MARGIN, gap
    plain, _, _ = hf_beam_search(oracle_step_fn(W, oc, embeds, nb, lora=lora), B, nb, V, N_NEW, eos, pad, process_fn(eos, OFF))
    acted(plain.tolist(), want.tolist(), eos, pad, checks)
    with with_eos(m32, eos), adapters(m32, lora):
        got, got_s = gen(m32, audio, video, dev, num_beams=nb, return_sequence_scores=True, **kw)
    assert torch.equal(got, want), (got, want)
    assert (got_s - want_s).abs().max() < 1e-5, (got_s, want_s)


def hf_keywords(kw):
    kw = dict(kw)
    if "sequence_bias" in kw:                                  # GenerationConfig's form: [[ids, bias], ...]
        kw["sequence_bias"] = [[list(k), v] for k, v in kw["sequence_bias"].items()]
    return kw


def test_pinned_to_transformers(dev, tiny, m32, embeds):  # noqa: F811
    """LlamaForCausalLM.generate(inputs_embeds=..., sequence_bias=..., bad_words_ids=..., suppress_tokens=..., begin_suppress_tokens=...)
    on the golden LLM weights (adapters off on both sides), greedy and beam search: its sequences equal the restatement's and generate()'s."""
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
    for nb, eos, kw in PINNED_CASES:
        with torch.no_grad():
            hf = llm.generate(inputs_embeds=embeds, attention_mask=mask, num_beams=nb, max_new_tokens=N_NEW, do_sample=False, eos_token_id=eos,
                              pad_token_id=pad, return_dict_in_generate=True, output_scores=True, num_return_sequences=1, **hf_keywords(kw))
        if nb == 1:
            want, margin = token_loop(oracle_step_fn(W, oc, embeds, 1, lora=False), B, N_NEW, eos, pad, process_fn(eos, full(kw)))
        else:
            want, want_s, margin = hf_beam_search(oracle_step_fn(W, oc, embeds, nb, lora=False), B, nb, V, N_NEW, eos, pad, process_fn(eos, full(kw)))
            assert (hf.sequences_scores - want_s).abs().max() < 1e-5
        assert margin > MARGIN, (nb, eos, kw, margin)
        assert torch.equal(hf.sequences, want), (nb, eos, kw, hf.sequences, want)
        with with_eos(m32, eos), m32.llm_engine.adapters_disabled():
            got = gen(m32, audio, video, dev, num_beams=nb, **kw)
        assert torch.equal(got, hf.sequences), (nb, eos, kw, got, hf.sequences)


# ------------------------------------------------------------------------------------------------ bf16 properties
MODES = {"greedy": {}, "sampled": dict(do_sample=True, temperature=1.0, top_k=20, top_p=0.9, seed=3), "beams": dict(num_beams=4)}


@pytest.mark.parametrize("decode_weights,B,fused", [("bf16", 2, True), ("bf16", 20, False), ("fp8", 2, True), ("fp4", 2, True)])
@pytest.mark.parametrize("mode", list(MODES))
def test_bf16_properties(dev, tiny, mode, decode_weights, B, fused):  # noqa: F811
    """On the fused and the general bf16 token step and on the fp8 and fp4 weight streams: the keywords at None change nothing; suppressed
    ids never occur; banned sequences never occur; a begin-suppressed token does not open a row."""
    from test_generate_processors_gpu import model16
    m = model16(tiny, decode_weights)
    a, v = batch(tiny, B)
    rows = B * (4 if mode == "beams" else 1)
    eng = m.llm_engine
    assert eng.decode_is_fused(rows) == fused
    assert eng.decode_streams_fp8(rows) == (decode_weights == "fp8") and eng.decode_streams_fp4(rows) == (decode_weights == "fp4")
    eos, pad = 53, m.tokenizer.pad_token_id
    kw = dict(MODES[mode], max_new_tokens=16)
    with with_eos(m, eos):
        plain = gen(m, a, v, dev, **kw)
        assert torch.equal(gen(m, a, v, dev, **OFF, hotwords=None, hotword_bias=0.0, **kw), plain)
        rows_plain = [trim(r, eos, pad) for r in plain.tolist()]
        # what the unprocessed output is made of: the first bigram and the first token of each row, and the other tokens
        bigrams = [list(b) for b in sorted({tuple(r[:2]) for r in rows_plain if len(r) >= 2 and eos not in r[:2]})]
        firsts = sorted({r[0] for r in rows_plain} - {eos})
        others = sorted({t for r in rows_plain for t in r} - {t for b in bigrams for t in b} - {eos})
        assert bigrams and firsts
        new = dict(suppress_tokens=others + [5, 5], bad_words_ids=bigrams + [[eos]], begin_suppress_tokens=firsts)
        got = gen(m, a, v, dev, **new, **kw)
        for r in got.tolist():
            r = trim(r, eos, pad)
            assert not set(r) & set(new["suppress_tokens"]), (r, new)
            assert not any(occurs([r], bg) for bg in bigrams), (r, bigrams)
            assert r[0] not in firsts, (r, firsts)
        if mode != "sampled":                               # the same rows in reverse order: rows do not depend on their neighbours
            back = gen(m, a.flip(0), v.flip(0), dev, **new, **kw)
            assert torch.equal(back.flip(0), got), (back.flip(0), got)


def test_bad_arguments_raise_before_any_gpu_work(dev, tiny, m32, monkeypatch):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    V = oc.llama.vocab

    class Reached(Exception):
        pass

    def no_gpu_work(*a, **k):
        raise Reached
    monkeypatch.setattr(m32, "_llm_inputs", no_gpu_work)
    many = {(i % 90 + 3, i // 90 + 3): 1.0 for i in range(4097)}
    bad = [dict(sequence_bias={}), dict(sequence_bias={(V,): 1.0}), dict(sequence_bias={(3,): 1}), dict(sequence_bias={(3,): float("inf")}),
           dict(sequence_bias={(): 1.0}), dict(sequence_bias={(3, -1): 1.0}), dict(sequence_bias=many), dict(sequence_bias={tuple(range(3, 20)): 1.0}),
           dict(bad_words_ids=[]), dict(bad_words_ids=[[]]), dict(bad_words_ids=[[V]]), dict(bad_words_ids=[[3.5]]), dict(bad_words_ids=[list(range(3, 20))]),
           dict(suppress_tokens=[V]), dict(suppress_tokens=[-1]), dict(suppress_tokens=[1.5]), dict(begin_suppress_tokens=[V]),
           dict(begin_suppress_tokens="3"), dict(hotwords="ab", hotword_bias=1.0), dict(hotwords=["ab"], hotword_bias=float("nan")),
           dict(hotwords=["ab"], hotword_bias=1.0, sequence_bias={(100,): 2.0}),            # "a" is token 100: a colliding key
           dict(sequence_bias={(3, 4): 1.0}, max_new_tokens=1025), dict(bad_words_ids=[[3, 4]], max_new_tokens=1025)]
    for kw in bad:
        for mode in MODES.values():
            with pytest.raises(ValueError):
                gen(m32, audio, video, dev, **dict(mode, **kw))
    # single-token tables need no history: the 1024-token limit does not apply to them
    for kw in (dict(suppress_tokens=[3]), dict(sequence_bias={(3,): 1.0}, bad_words_ids=[[4]], begin_suppress_tokens=[5])):
        for mode in MODES.values():
            with pytest.raises(Reached):
                gen(m32, audio, video, dev, **dict(mode, max_new_tokens=1025, **kw))
    with with_eos(m32, 4), pytest.raises(ValueError):          # [eos] is dropped, as HF drops it: nothing is left
        gen(m32, audio, video, dev, bad_words_ids=[[4]])


def test_decode_script_flags(dev, tmp_path):
    """decode.py --suppress_tokens / --begin_suppress_tokens / --bad_words / --hotwords / --hotword_bias: hypotheses made of the allowed
    alphabet only, the banned phrases in none, a hotword's first letter in some; the plain run shows neither."""
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

    plain = run("g")
    # restricting the vocabulary: everything but a-z, the space and EOS is suppressed (the byte tokenizer: id = byte + 3, EOS = 2)
    alphabet = "abcdefghijklmnopqrstuvwxyz "
    allowed = {ord(c) + 3 for c in alphabet} | {2}
    ids = tmp_path / "ids.txt"
    ids.write_text(" ".join(str(t) for t in range(512) if t not in allowed) + "\n")
    (tmp_path / "bad.txt").write_text("e\nth\n\n")
    (tmp_path / "hot.txt").write_text("zq\n")
    flags = ("--suppress_tokens", f"@{ids}", "--begin_suppress_tokens", "35,36", "--bad_words", str(tmp_path / "bad.txt"),
             "--hotwords", str(tmp_path / "hot.txt"), "--hotword_bias", "30")
    got = run("s", *flags)
    assert len(got) == 4 and got != plain and any(got)
    assert all(c in alphabet for h in got for c in h) and not all(c in alphabet for h in plain for c in h), (got, plain)
    assert not any("e" in h or "th" in h for h in got), got
    assert any("z" in h for h in got) and not any("z" in h for h in plain), (got, plain)        # the first token of a hotword's path is always boosted
