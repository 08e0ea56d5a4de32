"""generate() with decode_weights="fp8": greedy, sampling and beam search all run their token steps on the fp8 weight stream.  The yardstick
is built from public pieces: the bf16 prefill on the original weights, then the token steps of a bf16 engine whose weights are W~ (the
dequantised fp8 weights, tests/test_decode_fp8_gpu.py)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from avllm import ops  # noqa: E402
from test_decode_fp8_gpu import dequantised  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def _model(W, oc, with_lora=False, **kw):
    from avllm.arch import ClipCfg, LlamaCfg, LoraCfg, ModelCfg, WhisperCfg
    from avllm.model import ClipWhisperModel
    cfg = ModelCfg(WhisperCfg(**vars(oc.whisper)), ClipCfg(**vars(oc.clip)), LlamaCfg(**vars(oc.llama)), LoraCfg(oc.lora.r, oc.lora.alpha))
    return ClipWhisperModel(device="cuda:0", use_lora=with_lora, lora_r=oc.lora.r, lora_alpha=oc.lora.alpha, lora_dropout=0.0, max_seq_len=256,
                            config=cfg, weights=W, **kw).eval()


class _Hybrid:
    """prefill() of one engine (original bf16 weights), everything else -- decode_step() among it -- of another (W~)."""

    def __init__(self, prefill_eng, step_eng):
        self._p, self._s = prefill_eng, step_eng

    def prefill(self, *a, **k):
        return self._p.prefill(*a, **k)

    def __getattr__(self, name):
        return getattr(self._s, name)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    import numpy as np
    from oracle import weights as Wt
    g = np.load(f"{golden_dir}/g2_tiny_e2e.npz")
    oc = Wt.tiny()
    W = Wt.all_weights(oc, int(g["seed"]), lora_b_std=0.05)
    W = {k: v for k, v in W.items() if k != "lora"}
    audio, video, _, _ = Wt.synthetic_batch(oc, 4, int(g["frames"]), seed=int(g["batch_seed"]))
    return oc, W, audio.cuda(), video.cuda()


@pytest.fixture(scope="module")
def pair(dev, tiny):
    """(fp8-decode model, yardstick model): the yardstick is a bf16 model whose LLM prefills on W and steps on W~."""
    from avllm.engine import LlamaEngine
    oc, W, _, _ = tiny
    m8 = _model(W, oc, precision="bf16", decode_weights="fp8")
    ref = _model(W, oc, precision="bf16")
    et = LlamaEngine(dequantised(W["llama"]), ref.cfg.llama, None, None, dtype=BF, device=dev, training=False)
    ref.llm_engine = _Hybrid(ref.llm_engine, et)
    assert m8.llm_engine.decode_streams_fp8(4) and not ref.llm_engine.decode_streams_fp8(4)
    return m8, ref


def test_greedy_generate_fp8_matches_public_loop(dev, tiny, pair):
    oc, W, audio, video = tiny
    m8, ref = pair
    new = 24
    ids = m8.generate(audio=audio, video=video, max_new_tokens=new)
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
    thr = 1e-3                                                   # fp8 step vs bf16 step on W~: logits agree to ~1e-6 relative
    compared = 0
    for b in range(B):
        for t in range(min(got.shape[1], want.shape[1])):
            if int(want[b, t]) == m8.eos_token_id:
                break
            same = int(got[b, t]) == int(want[b, t])
            if float(margins[b, t]) >= thr:
                assert same, (b, t, got[b].tolist(), want[b].tolist())
                compared += 1
            elif not same:
                break
    assert compared >= 8, compared


def test_beam_and_sampled_generate_fp8_match_the_yardstick(dev, tiny, pair):
    oc, W, audio, video = tiny
    m8, ref = pair
    a, sa = m8.generate(audio=audio, video=video, max_new_tokens=12, num_beams=4, return_sequence_scores=True)
    b, sb = ref.generate(audio=audio, video=video, max_new_tokens=12, num_beams=4, return_sequence_scores=True)
    assert torch.equal(a, b)
    assert torch.allclose(sa, sb, rtol=0, atol=1e-4)
    a = m8.generate(audio=audio, video=video, max_new_tokens=12, do_sample=True, seed=1234)
    b = ref.generate(audio=audio, video=video, max_new_tokens=12, do_sample=True, seed=1234)
    assert torch.equal(a, b)


@pytest.mark.parametrize("precision", ["bf16", "fp8"])
def test_decode_weights_bf16_is_the_default(dev, tiny, precision):
    oc, W, audio, video = tiny
    a = _model(W, oc, precision=precision).generate(audio=audio, video=video, max_new_tokens=8)
    m = _model(W, oc, precision=precision, decode_weights="bf16")
    assert not m.llm_engine.decode_streams_fp8(4)
    assert torch.equal(a, m.generate(audio=audio, video=video, max_new_tokens=8))


def test_decode_weights_fp8_on_an_fp8_model_shares_the_codes(dev, tiny):
    """precision="fp8" + decode_weights="fp8": the token step streams the training forward's codes with the layout-2 exponents."""
    oc, W, audio, video = tiny
    m = _model(W, oc, precision="fp8", decode_weights="fp8")
    assert m.llm_engine.decode_streams_fp8(4)
    assert m.llm_engine.layers[0].wqkv8 and m.llm_engine.layers[0].eqkv8
    assert m.generate(audio=audio, video=video, max_new_tokens=4).shape == (4, 4)


def test_decode_weights_refusals(tiny):
    oc, W, _, _ = tiny
    with pytest.raises(ValueError):
        _model(W, oc, precision="fp32", decode_weights="fp8")
    with pytest.raises(ValueError):
        _model(W, oc, precision="bf16", decode_weights="int8")


def test_decode_py_with_fp8_decode_weights(dev, tmp_path):
    import glob
    data, dec = tmp_path / "toy", tmp_path / "dec"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_toy_dataset.py"), str(data)], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/clip_whisper/decode.py"), "--test_data", str(data / "test.tsv"),
                        "--test_wrd", str(data / "test.wrd"), "--output_dir", str(dec), "--modality", "both", "--batch_size", "2",
                        "--max_new_tokens", "4", "--tiny", "--data_path", str(data), "--decode_weights", "fp8"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Overall WER:" in r.stdout
    assert open(glob.glob(str(dec / "wer_*.txt"))[0]).read().split("\n")[1] == "Total samples: 4"
