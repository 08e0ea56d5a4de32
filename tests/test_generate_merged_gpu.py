"""ClipWhisperModel.merge_lora() on the tiny model of tests/refs64_merge.py (adapters large enough to matter, bf16 base) at max_seq_len 256.

  * the exported q/k/v/o weights are ops.lora_merge_ of the originals bit for bit and within the bar of merge64; every other LLM tensor is what
    went in;
  * the merged model runs the adapter-free kernels, and generates exactly what a use_lora=False model built from the exported weights generates
    (greedy, sampled, beam; bf16, fp8 and fp4 token-step weights, the fp8 cache, the fp8 training precision): both sides run the same kernels on the
    same bytes, so anything less than equality is a plumbing error -- an image not rebuilt, a pointer not cleared;
  * against the float64 reference WITH adapters it is inside the bf16 bars (tests/test_merge_refs_cpu.py shows that a merge which drops the term
    is three bars away);
  * everything that would need the separate adapters back raises, naming merge_lora; the adapters themselves stay in state_dict(), and a saved
    model reloads merged."""
import glob
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import generate_ref  # noqa: E402
import kv8_cases as K  # noqa: E402
import refs64_kv8 as R  # noqa: E402
import refs64_merge as M  # noqa: E402
from avllm import generation, ops  # noqa: E402
from bars import BF16_LOGITS_REL_L2, rel_l2  # noqa: E402
from bars_merge import merge_bar  # noqa: E402
from oracle import weights as Wt  # noqa: E402

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"bf16": dict(precision="bf16"), "fp8-steps": dict(precision="bf16", decode_weights="fp8"),
         "fp4-steps": dict(precision="bf16", decode_weights="fp4"), "fp8-steps-fp8-cache": dict(precision="bf16", decode_weights="fp8", kv_cache="fp8"),
         "fp8-precision": dict(precision="fp8")}


def _model(W=None, with_lora=True, **kw):
    from test_generate_fp8_gpu import _model as build
    oc, W0 = M.tiny()
    return build(W0 if W is None else W, oc, with_lora=with_lora, **kw)


def _plain_weights(exported):
    """M.tiny()'s weights without adapters and with the exported LLM (bf16 values as float32 on the CPU: the engine rounds them back unchanged)."""
    _, W0 = M.tiny()
    W = {k: v for k, v in W0.items() if k != "lora"}
    W["llama"] = {k: v.float().cpu() for k, v in exported.items()}
    return W


@pytest.fixture(scope="module")
def merged_bf16(dev):
    """(the merged bf16 model, its exported LLM, the use_lora=False model built from that)."""
    m = _model(precision="bf16")
    assert m.merge_lora() is m and m.llm_engine.merged and not m.training
    sd = m.merged_llm_state_dict()
    return m, sd, _model(_plain_weights(sd), with_lora=False, precision="bf16")


def test_exported_weights(dev, merged_bf16):
    oc, W = M.tiny()
    m, sd, _ = merged_bf16
    scale = oc.lora.scale
    assert m.llm_engine.lcfg.scale == scale and set(sd) == set(W["llama"])
    merged_keys = set()
    for i in range(oc.llama.layers):
        for nm in M.TARGETS:
            key = f"model.layers.{i}.self_attn.{nm}.weight"
            merged_keys.add(key)
            A, B = W["lora"][f"layers.{i}.{nm}.lora_A"], W["lora"][f"layers.{i}.{nm}.lora_B"]
            w0 = W["llama"][key].to(BF)
            assert sd[key].dtype == BF and sd[key].is_contiguous()
            assert torch.equal(sd[key], ops.lora_merge_(w0.to(dev), A.to(dev), B.to(dev), scale)), key
            ref, u, sum_abs = M.merge64(w0, A, B, scale)
            ratio = float(((sd[key].cpu().double() - ref).abs() / merge_bar(ref, u, sum_abs, A.shape[0], scale, True)).max())
            print(f"{key}: worst error / bar {ratio:.3f}; moved by {rel_l2(sd[key].cpu(), w0):.2e} relative L2")
            assert ratio <= 1.0 and not torch.equal(sd[key].cpu(), w0)
    for key, t in sd.items():
        if key not in merged_keys:
            assert torch.equal(t.cpu(), W["llama"][key].to(BF)), key
    sd["model.norm.weight"].zero_()                                    # clones: the engine does not see it
    assert torch.equal(m.merged_llm_state_dict()["model.norm.weight"].cpu(), W["llama"]["model.norm.weight"].to(BF))


def test_runs_the_adapter_free_path(dev, merged_bf16):
    m, _, plain = merged_bf16
    eng = m.llm_engine
    assert all(not ly.lora[j].A_pad and not ly.lora[j].B_pad for ly in eng.layers for j in range(4))
    assert all(not ly.wqkv_t and not ly.wo_t for ly in eng.layers), "the stale transposed copies are gone"
    assert eng.decode_is_fused(4) and plain.llm_engine.decode_is_fused(4)


@pytest.mark.parametrize("form", list(FORMS))
def test_generates_what_the_plain_model_generates(dev, merged_bf16, form):
    audio, video, _ = K.greedy_inputs()
    if form == "bf16":
        m, _, plain = merged_bf16
    else:
        m = _model(**FORMS[form])
        m.merge_lora()
        plain = _model(_plain_weights(m.merged_llm_state_dict()), with_lora=False, **FORMS[form])
    eng = m.llm_engine
    assert eng.decode_is_fused(4) and eng.decode_streams_fp8(4) == ("fp8-steps" in form) and eng.decode_streams_fp4(4) == (form == "fp4-steps")
    assert eng.decode_caches_fp8(4) == ("fp8-cache" in form)
    a, b = generate_ref.gen(m, audio, video, dev, K.N_GREEDY), generate_ref.gen(plain, audio, video, dev, K.N_GREEDY)
    assert torch.equal(a, b), "greedy"
    kw = dict(do_sample=True, seed=1234)
    assert torch.equal(generate_ref.gen(m, audio, video, dev, K.N_GREEDY, **kw), generate_ref.gen(plain, audio, video, dev, K.N_GREEDY, **kw)), "sampled"
    kw = dict(num_beams=4, return_sequence_scores=True)
    (ia, sa), (ib, sb) = generate_ref.gen(m, audio, video, dev, K.N_GREEDY, **kw), generate_ref.gen(plain, audio, video, dev, K.N_GREEDY, **kw)
    assert torch.equal(ia, ib) and torch.equal(sa, sb), "beam"
    with torch.no_grad():                                              # forward() in eval: the prefill kernels, every position
        fa, fb = (mm(audio=audio.to(dev), video=video.to(dev))["logits"] for mm in (m, plain))
    assert torch.equal(fa, fb)


def test_follows_the_adapter_reference(dev, merged_bf16):
    oc, W = M.tiny()
    m, _, _ = merged_bf16
    audio, video, x = K.greedy_inputs()
    sd, lora, c, lc = W["llama"], W["lora"], oc.llama, oc.lora
    eng = m.llm_engine
    kc, vc = eng.alloc_cache(x.shape[0], x.shape[1], fp8=False)
    _, full = eng.prefill(x.to(dev).to(BF), kc, vc, all_logits=True)
    e = rel_l2(full.float().cpu(), M.prefill_logits64(sd, lora, oc, x))
    print(f"merged prefill logits vs the float64 reference with adapters: relative L2 {e:.2e}")
    assert e < BF16_LOGITS_REL_L2
    ids = generate_ref.gen(m, audio, video, dev, K.N_GREEDY)
    ref, margins = R.greedy(sd, lora, c, lc, x, K.N_GREEDY, m.eos_token_id, m.tokenizer.pad_token_id, store=R.identity)
    held = R.held_decisions(ids, ref, margins, K.threshold())
    print(f"merged greedy: {held} decisions held")
    assert held >= K.MIN_HELD


def _engine_pair(dev, sd, cfg, lc, lora):
    from avllm.engine import LlamaEngine
    eng = LlamaEngine(sd, cfg, lc, lora, dtype=BF, device=dev, training=False)
    eng.merge_lora()
    plain = LlamaEngine({k: v.float().cpu() for k, v in eng.merged_llm_state_dict().items()}, cfg, None, None, dtype=BF, device=dev, training=False)
    return eng, plain


def _greedy(eng, x, vocab, n, dev):
    procs = generation.LogitsProcessors(vocab=vocab, eos=None, device=dev, max_new_tokens=n)
    return generation.token_loop(eng, x.to(dev).to(BF), None, 0, n, procs).cpu()


@pytest.mark.parametrize("name", ["q", "l"])
def test_attention_biases_merged_equals_plain(dev, name):
    """Qwen2 (q, k, v biases; d 896 over 2 kv heads: k and v are 128-row slices of wqkv) and a Llama with attention_bias (o as well): the biases
    are exported as they went in and the merged engine generates what the plain one does."""
    from avllm.arch import LoraCfg
    import attn_bias_weights as AW
    c = AW.CASES[name]
    sd, lora = AW.weights(c)
    eng, plain = _engine_pair(dev, sd, AW.llama_cfg(c), LoraCfg(AW.RANK, AW.ALPHA), lora)
    out = eng.merged_llm_state_dict()
    assert set(out) == set(sd) and all(torch.equal(out[k].cpu(), sd[k].to(BF)) for k in sd if k.endswith(".bias"))
    x = AW.batch(c)[0]
    a, b = _greedy(eng, x, c.vocab, AW.STEPS, dev), _greedy(plain, x, c.vocab, AW.STEPS, dev)
    assert torch.equal(a, b)


def test_qwen3_merged_equals_plain(dev):
    from avllm.arch import LoraCfg
    import qwen3_weights as QW
    c, sd, lora, x = K.qwen3_inputs()
    eng, plain = _engine_pair(dev, sd, QW.llama_cfg(c), LoraCfg(QW.RANK, QW.ALPHA), lora)
    out = eng.merged_llm_state_dict()
    assert set(out) == set(sd) and all(torch.equal(out[k].cpu(), sd[k].to(BF)) for k in sd if k.endswith("_norm.weight"))
    assert all(ly.q_norm_w for ly in eng.layers)
    a, b = _greedy(eng, x, c.vocab, K.QWEN3_NEW, dev), _greedy(plain, x, c.vocab, K.QWEN3_NEW, dev)
    assert torch.equal(a, b)


def test_refusals(dev, merged_bf16):
    oc, W = M.tiny()
    m, _, plain = merged_bf16
    audio, video, labels, prompt = Wt.synthetic_batch(oc, 2, 5, seed=7)
    with pytest.raises(RuntimeError, match="merge_lora"):
        m.merge_lora()
    assert not m.training
    m.train()
    try:
        with pytest.raises(RuntimeError, match="merge_lora"):
            m(audio=audio.to(dev), video=video.to(dev), prompt=prompt.to(dev), labels=labels.to(dev))
    finally:
        m.eval()
    state = m.state_dict()
    lora_keys = [k for k in state if "lora_" in k]
    assert len(lora_keys) == 8 * oc.llama.layers
    with pytest.raises(RuntimeError, match="merge_lora"):
        m.load_state_dict({k: state[k] for k in lora_keys})
    m.load_state_dict({k: v for k, v in state.items() if "connector" in k})          # connector tensors still load
    with pytest.raises(RuntimeError, match="merge_lora"):
        m.llm_engine.adapters_disabled()
    for call in (m.llm_engine.pack_lora, lambda: m.llm_engine.load_lora({}), lambda: m.llm_engine.fwd_loss(None, None), m.llm_engine.bwd):
        with pytest.raises(RuntimeError, match="merge_lora"):
            call()
    with pytest.raises(ValueError, match="merge_lora"):
        plain.merge_lora()
    with pytest.raises(RuntimeError, match="merge_lora"):
        plain.merged_llm_state_dict()
    # the adapters are still there, as loaded
    for k, v in W["lora"].items():
        _, i, mod, ab = k.split(".")
        assert torch.equal(state[f"llm.base_model.model.model.layers.{i}.self_attn.{mod}.{ab}.default.weight"].cpu(), v), k


def test_save_and_reload_merged(dev, merged_bf16, tmp_path):
    from avllm.arch import ClipCfg, LlamaCfg, LoraCfg, ModelCfg, WhisperCfg
    from avllm.model import ClipWhisperModel
    oc, W = M.tiny()
    m, _, _ = merged_bf16
    audio, video, _ = K.greedy_inputs()
    out_dir = str(tmp_path / "saved")
    m.save_pretrained(out_dir)
    W2 = dict(W)
    W2["lora"] = {k: torch.zeros_like(v) for k, v in W["lora"].items()}             # the adapters must come from the directory
    cfg = ModelCfg(WhisperCfg(**vars(oc.whisper)), ClipCfg(**vars(oc.clip)), LlamaCfg(**vars(oc.llama)), LoraCfg(oc.lora.r, oc.lora.alpha))
    m2 = ClipWhisperModel.from_pretrained(out_dir, merge_lora=True, device="cuda:0", config=cfg, weights=W2, precision="bf16", lora_dropout=0.0)
    assert m2.llm_engine.merged and not m2.training and m2.max_seq_len == m.max_seq_len
    assert torch.equal(generate_ref.gen(m2, audio, video, dev, K.N_GREEDY), generate_ref.gen(m, audio, video, dev, K.N_GREEDY))
    m3 = ClipWhisperModel.from_pretrained(out_dir, device="cuda:0", config=cfg, weights=W2, precision="bf16", lora_dropout=0.0)
    assert not m3.llm_engine.merged, "without the keyword nothing changes"


def test_decode_py_merge_lora(dev, tmp_path):
    data, dec = tmp_path / "toy", tmp_path / "dec"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_toy_dataset.py"), str(data)], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    common = [sys.executable, os.path.join(ROOT, "scripts/clip_whisper/decode.py"), "--test_data", str(data / "test.tsv"),
              "--test_wrd", str(data / "test.wrd"), "--output_dir", str(dec), "--modality", "both", "--batch_size", "2",
              "--max_new_tokens", "4", "--tiny", "--data_path", str(data)]
    r = subprocess.run(common + ["--load_lora", "--merge_lora"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Overall WER:" in r.stdout
    assert open(glob.glob(str(dec / "wer_*.txt"))[0]).read().split("\n")[1] == "Total samples: 4"
    assert "merged" in open(glob.glob(str(dec / "decode_*.log"))[0]).read()
    r = subprocess.run(common + ["--merge_lora"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and "--load_lora" in r.stderr
