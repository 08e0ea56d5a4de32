"""kv_cache="fp8" through the engine and through generate(): the prefill is the bf16 run's bit for bit and leaves the MX rule of its rows in the
cache, the fused token steps compute what tests/refs64_kv8.py computes on the same stored values, greedy / beam / scored generate() follow that
reference (greedy: the margin rule of test_decode_gpu.py; beam: the teacher-forced scores of test_generate_beam_gpu.py's bf16 tests -- at the bf16
threshold hf_beam_search's own selection gap is 1e-4 on these inputs, printed by tests/test_kv8_refs_cpu.py, so exact equality is asked only
where that gap allows it), and wherever the fused step does not apply, or the option is off, the results are the bf16 cache's byte for byte."""
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
from avllm import generation, ops  # noqa: E402
from avllm import lib as L  # noqa: E402
from bars import BF16_LOGIT_MAX_ABS, BF16_LOGITS_REL_L2, rel_l2  # noqa: E402
from generate_ref import with_eos  # noqa: E402
from oracle import mxfp8  # noqa: E402

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- engine
def _weights(hidden, heads, kvh, layers, ffn, vocab, seed=5):
    """test_decode_gpu._engine's draw, rounded to bf16 so that the engine and the float64 reference hold the same numbers."""
    from avllm.arch import LlamaCfg
    cfg = LlamaCfg(hidden, heads, layers, ffn, vocab)
    cfg.kv_heads = kvh
    g = torch.Generator().manual_seed(seed)
    dkv = kvh * (hidden // heads)
    sd = {"model.embed_tokens.weight": torch.randn(vocab, hidden, generator=g) * 0.5, "model.norm.weight": 1 + 0.1 * torch.randn(hidden, generator=g),
          "lm_head.weight": torch.randn(vocab, hidden, generator=g) * hidden ** -0.5}
    for i in range(layers):
        p = f"model.layers.{i}."
        for nm, (o, k) in {"self_attn.q_proj": (hidden, hidden), "self_attn.k_proj": (dkv, hidden), "self_attn.v_proj": (dkv, hidden),
                           "self_attn.o_proj": (hidden, hidden), "mlp.gate_proj": (ffn, hidden), "mlp.up_proj": (ffn, hidden),
                           "mlp.down_proj": (hidden, ffn)}.items():
            sd[p + nm + ".weight"] = torch.randn(o, k, generator=g) * k ** -0.5
        sd[p + "input_layernorm.weight"] = 1 + 0.1 * torch.randn(hidden, generator=g)
        sd[p + "post_attention_layernorm.weight"] = 1 + 0.1 * torch.randn(hidden, generator=g)
    return {k: v.to(BF).float() for k, v in sd.items()}, cfg


def _steps(eng, x, ids, S, new, B, device_pos=False):
    """prefill(S) + `new` token steps on a cache from eng.alloc_cache -> (prefill logits, step logits [B, new, V], K cache, V cache)."""
    dev = x.device
    kc, vc = eng.alloc_cache(B, S + new + 2)
    last, _ = eng.prefill(x[:, :S].contiguous(), kc, vc)
    pd = torch.zeros(1, device=dev, dtype=torch.int32) if device_pos else None
    outs = []
    for t in range(new):
        if device_pos:
            outs.append(eng.decode_step(ids[:, S + t].contiguous(), S, kc, vc, pos_dev=pd).clone())
            L.check(L.load().avllm_pos_advance(L.ptr(pd), 1, L.stream_ptr()))
        else:
            outs.append(eng.decode_step(ids[:, S + t].contiguous(), S + t, kc, vc).clone())
    return last, torch.stack(outs, 1), kc, vc


@pytest.mark.parametrize("hidden,heads,kvh,B", [(256, 2, 2, 3), (512, 8, 2, 8)])
def test_engine_token_steps_on_the_fp8_cache(dev, hidden, heads, kvh, B):
    from avllm.engine import LlamaEngine
    sd, cfg = _weights(hidden, heads, kvh, 2, 384, 256)
    e16 = LlamaEngine(sd, cfg, None, None, dtype=BF, device=dev, training=False)
    e8 = LlamaEngine(sd, cfg, None, None, dtype=BF, device=dev, training=False, kv_fp8=True)
    S, new, hd, dkv = 37, 4, hidden // heads, kvh * (hidden // heads)
    g = torch.Generator(device=dev).manual_seed(3)
    ids = torch.randint(0, cfg.vocab, (B, S + new), generator=g, device=dev)
    x = ops.embedding(e8.embed, ids.reshape(-1).contiguous()).view(B, S + new, hidden)
    assert e8.decode_caches_fp8(B) and e8.decode_is_fused(B) and not e16.decode_caches_fp8(B)
    last16, steps16, kc16, vc16 = _steps(e16, x, ids, S, new, B)
    last8, steps8, kc8, vc8 = _steps(e8, x, ids, S, new, B)
    assert kc8.dtype == torch.uint8 and kc16.dtype == BF
    assert kc8.numel() + vc8.numel() == e8.kv_cache_bytes(B, S + new + 2) == 2 * cfg.layers * B * (S + new + 2) * dkv * 33 // 32
    assert e16.kv_cache_bytes(B, S + new + 2) == 2 * kc16.numel() * 2
    assert torch.equal(last8, last16), "the prefill reads its own bf16 q|k|v: its logits are the bf16-cache run's"
    # after the prefill: the MX rule of the rows the bf16-cache engine holds, bit for bit; the reference starts from exactly these stored values
    past = []
    for c8, c16 in ((kc8, kc16), (vc8, vc16)):
        q, e = (t.cpu() for t in ops.kv8_unpack(c8))
        wq, we = mxfp8.quantize(c16[:, :, :S].float().cpu())
        assert torch.equal(q[:, :, :S], wq) and torch.equal(e[:, :, :S].int() - 127, we)
        past.append(R.mx_dequantize64(wq, we).view(cfg.layers, B, S, kvh, hd).transpose(2, 3))
    past = [(past[0][i], past[1][i]) for i in range(cfg.layers)]
    want = []
    with torch.no_grad():
        for t in range(new):
            h = R.llama_hidden(sd, None, cfg, None, sd["model.embed_tokens.weight"][ids[:, S + t].cpu()][:, None], past, S + t)
            want.append(h[:, -1] @ sd["lm_head.weight"].double().T)
    want = torch.stack(want, 1)
    e = rel_l2(steps8.cpu(), want)
    print(f"fp8-cache token steps vs refs64_kv8 on the same stored rows: relative L2 {e:.2e}; vs the bf16-cache steps {rel_l2(steps8, steps16):.2e}")
    assert e < BF16_LOGITS_REL_L2
    assert torch.equal(_steps(e8, x, ids, S, new, B, device_pos=True)[1], steps8)            # the position merely comes from memory
    # the general path (the fused one switched off) gets the bf16 cache and computes what an engine without the option computes
    with L.knob("DECODE_FUSED", 0):
        assert not e8.decode_caches_fp8(B)
        l8, s8, k8, _ = _steps(e8, x, ids, S, new, B)
        l16, s16, _, _ = _steps(e16, x, ids, S, new, B)
    assert k8.dtype == BF and torch.equal(l8, l16) and torch.equal(s8, s16)


def test_engine_more_than_16_rows_keep_the_bf16_cache(dev):
    from avllm.engine import LlamaEngine
    sd, cfg = _weights(256, 2, 2, 2, 384, 256)
    e16 = LlamaEngine(sd, cfg, None, None, dtype=BF, device=dev, training=False)
    e8 = LlamaEngine(sd, cfg, None, None, dtype=BF, device=dev, training=False, kv_fp8=True)
    B, S, new = 17, 9, 2
    g = torch.Generator(device=dev).manual_seed(4)
    ids = torch.randint(0, cfg.vocab, (B, S + new), generator=g, device=dev)
    x = ops.embedding(e8.embed, ids.reshape(-1).contiguous()).view(B, S + new, 256)
    assert e8.decode_caches_fp8(16) and not e8.decode_caches_fp8(17)
    l8, s8, k8, _ = _steps(e8, x, ids, S, new, B)
    l16, s16, _, _ = _steps(e16, x, ids, S, new, B)
    assert k8.dtype == BF and torch.equal(l8, l16) and torch.equal(s8, s16)
    # a cache in the wrong form for the step is refused, not reinterpreted
    kc, vc = e8.alloc_cache(B, S + 2, fp8=True)
    e8.prefill(x[:, :S].contiguous(), kc, vc)
    with pytest.raises(ValueError, match="kv_fp8"):
        e8.decode_step(ids[:, S].contiguous(), S, kc, vc)
    with pytest.raises(ValueError, match="kv_fp8"):
        e16.prefill(x[:, :S].contiguous(), kc, vc)
    with pytest.raises(ValueError, match="kv_fp8"):
        LlamaEngine(sd, cfg, None, None, dtype=torch.float32, device=dev, training=False, kv_fp8=True)


def test_engine_qwen3_head_norms_through_the_token_loop(dev):
    """Qwen3 case "a" (tests/qwen3_weights.py), adapters on: generate()'s own loop (generation.token_loop) on an engine with the fp8 cache -- the
    head-norm launch rotates in place, the append follows without rotating again -- followed against the reference by the margin rule."""
    from avllm.arch import LoraCfg
    from avllm.engine import LlamaEngine
    import qwen3_weights as QW
    c, sd, lora, x = K.qwen3_inputs()
    lc = LoraCfg(QW.RANK, QW.ALPHA)
    eng = LlamaEngine(sd, QW.llama_cfg(c), lc, lora, dtype=BF, device=dev, training=False, kv_fp8=True)
    assert eng.decode_caches_fp8(x.shape[0]) and all(ly.q_norm_w for ly in eng.layers)
    procs = generation.LogitsProcessors(vocab=c.vocab, eos=None, device=dev, max_new_tokens=K.QWEN3_NEW)
    ids = generation.token_loop(eng, x.to(dev).to(BF), None, 0, K.QWEN3_NEW, procs).cpu()
    ref, margins = R.greedy(sd, lora, c, lc, x, K.QWEN3_NEW, None, 0)
    held = R.held_decisions(ids, ref, margins, K.threshold())
    print(f"Qwen3 fp8 cache: {held} decisions held")
    assert held >= K.MIN_HELD


# ---------------------------------------------------------------- model
def _model(with_lora=True, **kw):
    from test_generate_fp8_gpu import _model as build
    oc, W, _, _ = K.tiny(with_lora)
    return build(W, oc, with_lora=with_lora, precision="bf16", **kw)


@pytest.mark.parametrize("case", ["plain", "adapters", "fp8-weights"])
def test_greedy_generate_follows_the_reference(dev, case):
    with_lora = case == "adapters"
    kw = {"decode_weights": "fp8"} if case == "fp8-weights" else {}
    oc, W, _, _ = K.tiny(with_lora)
    audio, video, x = K.greedy_inputs()
    m8, m16 = _model(with_lora, kv_cache="fp8", **kw), _model(with_lora, **kw)
    assert m8.kv_cache == "fp8" and m8.llm_engine.decode_caches_fp8(4) and not m16.llm_engine.decode_caches_fp8(4)
    assert m8.eos_token_id == 2
    ids8 = generate_ref.gen(m8, audio, video, dev, K.N_GREEDY)
    ids16 = generate_ref.gen(m16, audio, video, dev, K.N_GREEDY)
    assert torch.equal(ids8[:, 0], ids16[:, 0]), "the prefill, so the first token, is the bf16-cache run's"
    steps = None
    if case == "fp8-weights":
        from test_decode_fp8_gpu import dequantised
        steps = dequantised(W["llama"])
    ref, margins = R.greedy(W["llama"], W.get("lora"), oc.llama, oc.lora, x, K.N_GREEDY, m8.eos_token_id, m8.tokenizer.pad_token_id, sd_steps=steps)
    held = R.held_decisions(ids8, ref, margins, K.threshold())
    print(f"greedy kv_cache=fp8 ({case}): {held} decisions held; tokens equal to the bf16-cache run: {int((ids8[:, :ids16.shape[1]] == ids16[:, :ids8.shape[1]]).sum())}")
    assert held >= K.MIN_HELD


def test_beam_search_scores_are_the_references(dev):
    """num_beams = 3 on 2 items: 6 rows through the prefix broadcast and the per-step reorder of the image.  Each returned score is the reference's
    teacher-forced mean log-probability of that hypothesis within 2 x the bf16 logit bar (a step's log-probability moves by the logit's error and
    by the normaliser's), and not below the greedy hypothesis' by more than that; the sequences are hf_beam_search's where its closest selection
    edge is further apart than the threshold."""
    oc, W, _, _ = K.tiny()
    sd, lora, c, lc = W["llama"], W["lora"], oc.llama, oc.lora
    audio, video, x = K.beam_inputs()
    m = _model(True, kv_cache="fp8")
    assert m.llm_engine.decode_caches_fp8(K.BEAM_B * K.BEAM_NB)
    pad = m.tokenizer.pad_token_id
    with with_eos(m, K.BEAM_EOS):
        ids, scores = generate_ref.gen(m, audio, video, dev, K.BEAM_N, num_beams=K.BEAM_NB, return_sequence_scores=True)
        greedy = generate_ref.gen(m, audio, video, dev, K.BEAM_N)
    tot, lens, _ = R.forced(sd, lora, c, lc, x, ids, K.BEAM_EOS)
    tol = 2.0 * BF16_LOGIT_MAX_ABS
    print(f"beam kv_cache=fp8: scores {scores.tolist()}, reference along the same hypotheses {(tot / lens.double()).tolist()}")
    assert ((scores.double() - tot / lens.double()).abs() <= tol).all()
    gt, gl, _ = R.forced(sd, lora, c, lc, x, greedy, K.BEAM_EOS)
    assert (scores.double() >= gt / gl.double() - tol).all()
    want, want_s, gap = generate_ref.hf_beam_search(R.step_fn(sd, lora, c, lc, x, K.BEAM_NB), K.BEAM_B, K.BEAM_NB, c.vocab, K.BEAM_N, K.BEAM_EOS, pad)
    print(f"hf_beam_search on the reference: closest selection edge {gap:.4f} (threshold {K.threshold()}), same sequences: {torch.equal(ids, want)}")
    if gap >= K.threshold():
        assert torch.equal(ids, want)


def test_eighteen_rows_and_the_default_are_the_bf16_cache(dev):
    audio, video, _ = K.beam_inputs()
    m8, m16, mdef = _model(True, kv_cache="fp8"), _model(True, kv_cache="bf16"), _model(True)
    assert mdef.kv_cache == "bf16" and not mdef.llm_engine.kv_fp8 and mdef.llm_engine.desc.kv_fp8 == 0
    assert not mdef.llm_engine.decode_caches_fp8(1) and mdef.llm_engine.alloc_cache(2, 4)[0].dtype == BF
    # 2 items x 9 beams = 18 rows: the general step, the bf16 cache, the same bytes
    assert not m8.llm_engine.decode_caches_fp8(18)
    a = generate_ref.gen(m8, audio, video, dev, 5, num_beams=9, return_sequence_scores=True)
    b = generate_ref.gen(m16, audio, video, dev, 5, num_beams=9, return_sequence_scores=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the default: byte-equal outputs with and without the keyword, greedy and beam, and forward() alike with the option on
    for kw in ({}, {"num_beams": 3, "return_sequence_scores": True}):
        a, b = generate_ref.gen(mdef, audio, video, dev, 6, **kw), generate_ref.gen(m16, audio, video, dev, 6, **kw)
        assert all(torch.equal(s, t) for s, t in zip(a, b)) if isinstance(a, tuple) else torch.equal(a, b)
    with torch.no_grad():
        f8, f16 = m8(audio=audio.to(dev), video=video.to(dev)), m16(audio=audio.to(dev), video=video.to(dev))
    assert torch.equal(f8["logits"], f16["logits"]), "forward()'s eval path keeps its bf16 cache"


def test_token_scores_run_and_start_as_the_bf16_cache(dev):
    audio, video, _ = K.beam_inputs()
    m8, m16 = _model(True, kv_cache="fp8"), _model(True)
    o8 = m8.generate(audio=audio.to(dev), video=video.to(dev), max_new_tokens=6, return_token_scores=True)
    o16 = m16.generate(audio=audio.to(dev), video=video.to(dev), max_new_tokens=6, return_token_scores=True)
    assert o8.sequences.shape == o8.token_scores.shape == o8.token_entropy.shape and bool(torch.isfinite(o8.token_scores).all())
    assert torch.equal(o8.token_scores[:, 0], o16.token_scores[:, 0]) and torch.equal(o8.token_entropy[:, 0], o16.token_entropy[:, 0])
    assert bool((o8.token_scores <= 0).all())
    s8 = m8.generate(audio=audio.to(dev), video=video.to(dev), max_new_tokens=6, do_sample=True, top_k=1, seed=1)
    assert torch.equal(s8, o8.sequences), "sampling with top_k = 1 is the greedy run on the same steps"


def test_refusals(dev):
    with pytest.raises(ValueError, match=r"kv_cache.*precision|precision.*kv_cache"):
        from test_generate_fp8_gpu import _model as build
        oc, W, _, _ = K.tiny()
        build(W, oc, with_lora=True, precision="fp32", kv_cache="fp8")
    with pytest.raises(ValueError, match="kv_cache"):
        _model(True, kv_cache="int8")


def test_decode_py_with_the_fp8_cache(dev, tmp_path):
    data, dec = tmp_path / "toy", tmp_path / "dec"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_toy_dataset.py"), str(data)], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/clip_whisper/decode.py"), "--test_data", str(data / "test.tsv"),
                        "--test_wrd", str(data / "test.wrd"), "--output_dir", str(dec), "--modality", "both", "--batch_size", "2",
                        "--max_new_tokens", "4", "--tiny", "--data_path", str(data), "--kv_cache", "fp8"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Overall WER:" in r.stdout
    assert open(glob.glob(str(dec / "wer_*.txt"))[0]).read().split("\n")[1] == "Total samples: 4"
    assert glob.glob(str(dec / "decode_results.json"))
