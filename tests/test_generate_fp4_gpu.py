"""generate() with decode_weights="fp4": greedy, sampling, beam search and the logits processors all run their token steps on the MXFP4 weight
stream.  The yardstick is built from public pieces, as for fp8 (tests/test_generate_fp8_gpu.py): the bf16 prefill on the original weights W,
then the token steps of a bf16 engine whose weights are W~ (projections through mxfp4_ref, lm_head through the e4m3 rule)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from avllm import ops  # noqa: E402
from test_decode_fp4_gpu import dequantised4  # noqa: E402
from test_generate_fp8_gpu import _Hybrid, _model, tiny  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


@pytest.fixture(scope="module")
def pair(dev, tiny):
    """(fp4-decode model, yardstick model): the yardstick is a bf16 model whose LLM prefills on W and steps on W~."""
    from avllm.engine import LlamaEngine
    oc, W, _, _ = tiny
    m4 = _model(W, oc, precision="bf16", decode_weights="fp4")
    ref = _model(W, oc, precision="bf16")
    et = LlamaEngine(dequantised4(W["llama"]), ref.cfg.llama, None, None, dtype=BF, device=dev, training=False)
    ref.llm_engine = _Hybrid(ref.llm_engine, et)
    assert m4.llm_engine.decode_streams_fp4(4) and not m4.llm_engine.decode_streams_fp8(4) and not ref.llm_engine.decode_streams_fp4(4)
    return m4, ref


def test_greedy_generate_fp4_matches_public_loop(dev, tiny, pair):
    oc, W, audio, video = tiny
    m4, ref = pair
    new = 32
    ids = m4.generate(audio=audio, video=video, max_new_tokens=new)
    # the loop from public pieces, with the top-2 margin of every step
    x = ref._llm_inputs(audio, video, None)
    eng = ref.llm_engine
    B, S, _ = x.shape
    kc, vc = eng.alloc_cache(B, S + new)
    logits, _ = eng.prefill(x, kc, vc)
    toks, margins = [], []
    for t in range(new):
        top = logits.topk(2, -1).values
        margins.append(top[:, 0] - top[:, 1])
        nxt = ops.argmax_rows(logits)
        toks.append(nxt)
        logits = eng.decode_step(nxt, S + t, kc, vc)
    want, margins = torch.stack(toks, 1).cpu(), torch.stack(margins, 1).cpu()
    got = ids.cpu()
    thr = 1e-3                                                   # fp4 step vs bf16 step on W~: the same products, another fp32 grouping
    compared = 0
    for b in range(B):
        for t in range(min(got.shape[1], want.shape[1])):
            if int(want[b, t]) == m4.eos_token_id:
                break
            same = int(got[b, t]) == int(want[b, t])
            if float(margins[b, t]) >= thr:
                assert same, (b, t, got[b].tolist(), want[b].tolist())
                compared += 1
            elif not same:
                break
    print(f"greedy fp4: {compared} tokens compared")
    assert compared >= 8, compared


def test_beam_and_sampled_generate_fp4_match_the_yardstick(dev, tiny, pair):
    oc, W, audio, video = tiny
    m4, ref = pair
    a, sa = m4.generate(audio=audio, video=video, max_new_tokens=12, num_beams=4, return_sequence_scores=True)
    b, sb = ref.generate(audio=audio, video=video, max_new_tokens=12, num_beams=4, return_sequence_scores=True)
    assert torch.equal(a, b)
    assert torch.allclose(sa, sb, rtol=0, atol=1e-4)
    a = m4.generate(audio=audio, video=video, max_new_tokens=12, do_sample=True, seed=1234)
    b = ref.generate(audio=audio, video=video, max_new_tokens=12, do_sample=True, seed=1234)
    assert torch.equal(a, b)


def test_logits_processors_on_the_fp4_step_match_the_yardstick(dev, tiny, pair):
    oc, W, audio, video = tiny
    m4, ref = pair
    kw = dict(audio=audio, video=video, max_new_tokens=12, repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert torch.equal(m4.generate(**kw), ref.generate(**kw))


def test_decode_weights_default_is_untouched_by_fp4(dev, tiny):
    """decode_weights left alone: no fp4 image is built, no fp4 step is taken, and the output is what decode_weights="bf16" gives."""
    oc, W, audio, video = tiny
    m0 = _model(W, oc, precision="bf16")
    m = _model(W, oc, precision="bf16", decode_weights="bf16")
    for x in (m0, m):
        assert not x.llm_engine.decode_streams_fp4(4) and not x.llm_engine.decode_fp4 and not x.llm_engine.layers[0].wqkv4
    assert torch.equal(m0.generate(audio=audio, video=video, max_new_tokens=8), m.generate(audio=audio, video=video, max_new_tokens=8))


def test_decode_weights_fp4_on_an_fp8_model(dev, tiny):
    """precision="fp8" + decode_weights="fp4": the training forward keeps its e4m3 images, the token step streams the MXFP4 ones."""
    oc, W, audio, video = tiny
    m = _model(W, oc, precision="fp8", decode_weights="fp4")
    ly = m.llm_engine.layers[0]
    assert m.llm_engine.decode_streams_fp4(4) and ly.wqkv8 and ly.sqkv8 and ly.wqkv4 and ly.eqkv4
    assert m.generate(audio=audio, video=video, max_new_tokens=4).shape == (4, 4)


def test_fp4_refusals_and_use_4bit(dev, tiny):
    oc, W, _, _ = tiny
    with pytest.raises(ValueError):
        _model(W, oc, precision="fp32", decode_weights="fp4")
    with pytest.raises(ValueError):
        _model(W, oc, precision="bf16", decode_weights="nf4")
    with pytest.raises(NotImplementedError):
        _model(W, oc, precision="bf16", use_4bit=True)           # bitsandbytes NF4 stays refused: decode_weights="fp4" is not that mode
    with pytest.raises(NotImplementedError):
        _model(W, oc, precision="bf16", use_4bit=True, decode_weights="fp4")


def test_decode_py_with_fp4_decode_weights(dev, tmp_path):
    import glob
    data, dec = tmp_path / "toy", tmp_path / "dec"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_toy_dataset.py"), str(data)], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/clip_whisper/decode.py"), "--test_data", str(data / "test.tsv"),
                        "--test_wrd", str(data / "test.wrd"), "--output_dir", str(dec), "--modality", "both", "--batch_size", "2",
                        "--max_new_tokens", "4", "--tiny", "--data_path", str(data), "--decode_weights", "fp4"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Overall WER:" in r.stdout
    assert open(glob.glob(str(dec / "wer_*.txt"))[0]).read().split("\n")[1] == "Total samples: 4"
