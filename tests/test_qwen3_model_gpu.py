"""Qwen3's per-head q/k RMSNorm through every LLM path, on the g13 fixtures (tools/make_golden_qwen3.py: transformers' Qwen3ForCausalLM with
peft-style adapters, CPU fp32): training forward / backward in fp32, bf16 and fp8, prefill, the general token step, and the fused token step
(raw q|k|v projection + avllm_qk_norm_rope in its cache form) in its bf16, fp8 and fp4 weight forms.  Test for test the shape of
tests/test_attn_bias_model_gpu.py; the engine is driven directly (LlamaEngine).  Bars: tests/bars.py, unchanged."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import qwen3_weights as QW  # noqa: E402
from bars import rel_l2  # noqa: E402

BF = torch.bfloat16
S, STEPS = QW.S, QW.STEPS
# the bar of tests/test_attn_bias_model_gpu.py (and of the two tests that define the comparison: test_decode_fp8_gpu.py, test_decode_fp4_gpu.py)
# for a whole token step in a code form against the bf16 step on the dequantised weights: half of BF16_LOGITS_REL_L2
TOKEN_STEP_CODE_FORM_REL_L2 = 0.5 * Bar.BF16_LOGITS_REL_L2


@pytest.fixture(scope="module")
def cases(golden_dir):
    out = {}
    for name, c in QW.CASES.items():
        z = np.load(os.path.join(golden_dir, QW.golden_name(c)))
        gold = {k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files}
        sd, lora = QW.weights(c)
        out[name] = (c, QW.llama_cfg(c), sd, lora, gold)
    return out


def engine(dev, cfg, sd, lora, dtype, training=True, **kw):
    from avllm.arch import LoraCfg
    from avllm.engine import LlamaEngine
    return LlamaEngine(sd, cfg, LoraCfg(QW.RANK, QW.ALPHA) if lora is not None else None, lora, dtype=dtype, device=dev, training=training, **kw)


def ops_knob(name, value):
    from avllm import lib as L
    return L.knob(name, value)


def train_step(eng, gold, dev):
    """-> (logits, loss, {LoRA gradient}, dx_embeds) of one forward / backward on the fixture's batch."""
    x, labels = gold["inputs_embeds"].to(dev, eng.dtype), gold["labels"].to(dev)
    logits = eng.fwd_loss(x, labels, want_logits=True)
    eng.lora_g.zero_()
    dx = torch.empty_like(x)
    eng.bwd(dx_embeds=dx)
    torch.cuda.synchronize()
    loss = float(eng.acc[0] / eng.acc[1])
    return logits.float().cpu(), loss, {k: v.clone().cpu() for k, v in eng.lora_views(eng.lora_g).items()}, dx.float().cpu()


def forced_steps(eng, gold, dev, rows=QW.B):
    """The eight token steps teacher-forced on the fixture's tokens: [rows, STEPS, vocab] f32.  Step 0 is the prefill's last position; `rows`
    tiles the fixture's two sequences (row i = sequence i % 2)."""
    idx = torch.arange(rows) % QW.B
    x = gold["inputs_embeds"][idx].to(dev, eng.dtype)
    toks = gold["tokens"][idx].to(dev)
    kc, vc = eng.alloc_cache(rows, S + STEPS)
    out = [eng.prefill(x, kc, vc)[0].clone()]
    for t in range(1, STEPS):
        out.append(eng.decode_step(toks[:, t - 1].contiguous(), S + t - 1, kc, vc).clone())
    return torch.stack(out, 1).float().cpu()


# ------------------------------------------------------------------------------------------------ fp32
@pytest.mark.parametrize("name", ["a", "b"])
def test_fp32_matches_transformers(dev, cases, name):
    c, cfg, sd, lora, gold = cases[name]
    eng = engine(dev, cfg, sd, lora, torch.float32)
    logits, loss, grads, dx = train_step(eng, gold, dev)
    dl = float((logits - gold["logits"]).abs().max())
    print(f"{name} fp32: max |dlogits| {dl:.2e}, |dloss| {abs(loss - float(gold['loss'])):.2e}")
    assert dl < Bar.F32_LOGITS_ABS
    assert abs(loss - float(gold["loss"])) < Bar.F32_LOSS_ABS
    for k, g in grads.items():
        ref = gold["grad." + k]
        assert float((g - ref).abs().max()) <= Bar.F32_GRAD_REL_MAX * float(ref.abs().max()), k
    assert float((dx - gold["dx_embeds"]).abs().max()) <= Bar.F32_GRAD_REL_MAX * float(gold["dx_embeds"].abs().max())
    # greedy: prefill + seven token steps, each fed its own argmax
    x = gold["inputs_embeds"].to(dev)
    kc, vc = eng.alloc_cache(QW.B, S + STEPS)
    step = eng.prefill(x, kc, vc)[0]
    for t in range(STEPS):
        assert float((step.cpu() - gold["step_logits"][:, t]).abs().max()) < Bar.F32_LOGITS_ABS, t
        tok = step.argmax(-1)
        assert torch.equal(tok.cpu(), gold["tokens"][:, t]), t
        if t + 1 < STEPS:
            step = eng.decode_step(tok.contiguous(), S + t, kc, vc)
    with eng.adapters_disabled():
        base = forced_steps(eng, gold, dev)
    assert float((base - gold["step_logits_base"]).abs().max()) < Bar.F32_LOGITS_ABS


@pytest.mark.parametrize("what", ["unit", "swapped", "dropped"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_other_norms_are_another_model(dev, cases, name, what):
    """Negative controls: the norm weights replaced by ones (a kernel that skips the weight), q's and k's vectors swapped, and the same state
    dict run as qk_norm=False with the keys dropped (no norm at all) each miss the fp32 logits bar by more than 10 x, in the training forward and
    in the token steps."""
    c, cfg, sd, lora, gold = cases[name]
    if what == "dropped":
        eng = engine(dev, QW.llama_cfg(c, qk_norm=False), QW.without_norms(sd), lora, torch.float32, training=False)
    else:
        eng = engine(dev, cfg, (QW.with_unit_norms if what == "unit" else QW.with_swapped_norms)(sd), lora, torch.float32, training=False)
    x, labels = gold["inputs_embeds"].to(dev), gold["labels"].to(dev)
    logits = eng.fwd_loss(x, labels, want_logits=True).float().cpu()
    dl = float((logits - gold["logits"]).abs().max())
    ds = float((forced_steps(eng, gold, dev) - gold["step_logits"]).abs().max())
    print(f"{name}: norms {what}: max |dlogits| {dl:.3f} (forward), {ds:.3f} (token steps), rel L2 {rel_l2(logits, gold['logits']):.3f}")
    assert dl > 10 * Bar.F32_LOGITS_ABS and ds > 10 * Bar.F32_LOGITS_ABS


# ------------------------------------------------------------------------------------------------ bf16
@pytest.mark.parametrize("name", ["a", "b"])
def test_bf16_training_step(dev, cases, name):
    c, cfg, sd, lora, gold = cases[name]
    eng = engine(dev, cfg, sd, lora, BF)
    logits, loss, grads, dx = train_step(eng, gold, dev)
    keys = sorted(grads)
    e_l, e_g = rel_l2(logits, gold["logits"]), rel_l2(torch.cat([grads[k].flatten() for k in keys]), torch.cat([gold["grad." + k].flatten() for k in keys]))
    e_x = rel_l2(dx, gold["dx_embeds"])
    print(f"{name} bf16: logits {e_l:.3e}, |dloss| {abs(loss - float(gold['loss'])):.3e}, LoRA grads {e_g:.3e}, dx_embeds {e_x:.3e}")
    assert e_l < Bar.BF16_LOGITS_REL_L2
    assert abs(loss - float(gold["loss"])) < Bar.BF16_LOSS_ABS
    assert e_g < Bar.BF16_GRAD_REL_L2 and e_x < Bar.BF16_GRAD_REL_L2


@pytest.mark.parametrize("name", ["a", "b"])
def test_bf16_token_steps_fused_and_general(dev, cases, name):
    c, cfg, sd, lora, gold = cases[name]
    eng = engine(dev, cfg, sd, lora, BF, training=False)
    assert eng.decode_is_fused(QW.B) and not eng.decode_is_fused(17)
    got = forced_steps(eng, gold, dev)
    for t in range(STEPS):
        e = rel_l2(got[:, t], gold["step_logits"][:, t])
        print(f"{name} bf16 fused step {t}: {e:.3e}")
        assert e < Bar.BF16_LOGITS_REL_L2, t
    with eng.adapters_disabled():
        assert eng.decode_is_fused(QW.B)
        base = forced_steps(eng, gold, dev)
    for t in range(STEPS):
        assert rel_l2(base[:, t], gold["step_logits_base"][:, t]) < Bar.BF16_LOGITS_REL_L2, t
    wide = forced_steps(eng, gold, dev, rows=17)                      # 17 rows: the general path (avllm_qk_norm_rope in place + kv_append)
    want = gold["step_logits"][torch.arange(17) % QW.B]
    for t in range(STEPS):
        assert rel_l2(wide[:, t], want[:, t]) < Bar.BF16_LOGITS_REL_L2, t
    with ops_knob("DECODE_FUSED", 0):                                # and the general path at the fixture's own two rows
        assert not eng.decode_is_fused(QW.B)
        gen = forced_steps(eng, gold, dev)
    for t in range(STEPS):
        assert rel_l2(gen[:, t], gold["step_logits"][:, t]) < Bar.BF16_LOGITS_REL_L2, t


# ------------------------------------------------------------------------------------------------ fp8 / fp4
@pytest.mark.parametrize("name", ["a", "b"])
def test_fp8_training_forward(dev, cases, name):
    """precision fp8: the frozen products run on the e4m3 images, the head norm and RoPE on their bf16 output.  Held to the project's bar for
    fp8 against the unquantised arithmetic of the same model, here the bf16 run; the loss difference is printed."""
    c, cfg, sd, lora, gold = cases[name]
    x, labels = gold["inputs_embeds"].to(dev, BF), gold["labels"].to(dev)
    e16, e8 = engine(dev, cfg, sd, lora, BF), engine(dev, cfg, sd, lora, BF, fp8=True)
    l16 = e16.fwd_loss(x, labels, want_logits=True).float().cpu()
    loss16 = float(e16.acc[0] / e16.acc[1])
    l8 = e8.fwd_loss(x, labels, want_logits=True).float().cpu()
    loss8 = float(e8.acc[0] / e8.acc[1])
    e8.lora_g.zero_()
    e8.bwd()
    torch.cuda.synchronize()
    cost = rel_l2(l8, l16)
    print(f"{name} fp8 forward vs bf16: logits {cost:.3e}, loss {loss8:.4f} vs {loss16:.4f}; vs the fixture {rel_l2(l8, gold['logits']):.3e}")
    assert torch.isfinite(l8).all() and torch.isfinite(e8.lora_g).all()
    assert cost < Bar.FP8_VS_UNQUANTISED_REL_L2
    # and against the float64 step with the frozen products fake-quantised (tests/refs64_lora_mlp.py fp8_proj, tied to the oracle's fp8 mode by
    # tests/test_train_step_cases_cpu.py), on the bf16 values the engine holds: logits, loss and the adapter gradients at the fp8 bars
    import refs64_lora_mlp as R64
    as_held = lambda t: {k: v.bfloat16().float() for k, v in t.items()}      # noqa: E731
    rl, rlogits, rg, _ = R64.step(as_held(sd), as_held(lora), c, QW.ALPHA / QW.RANK, gold["inputs_embeds"], gold["labels"], proj=R64.fp8_proj)
    g8 = {k: v.cpu() for k, v in e8.lora_views(e8.lora_g).items()}
    keys = sorted(rg)
    e_l, e_g = rel_l2(l8, rlogits), rel_l2(torch.cat([g8[k].flatten() for k in keys]), torch.cat([rg[k].flatten() for k in keys]))
    print(f"{name} fp8 vs the fake-quantised float64 step: logits {e_l:.3e}, |dloss| {abs(loss8 - float(rl)):.3e}, LoRA grads {e_g:.3e}")
    assert set(g8) == set(rg)
    assert e_l < Bar.FP8_LOGITS_REL_L2 and abs(loss8 - float(rl)) < Bar.FP8_LOSS_ABS and e_g < Bar.FP8_GRAD_REL_L2


@pytest.mark.parametrize("form", ["fp8", "fp4"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_weight_only_token_steps(dev, cases, name, form):
    """decode_weights fp8 | fp4: the fused step streams the codes into the raw q|k|v projection, the head norm follows.  Bar: the project's
    figure for the code forms against the bf16 step on the dequantised weights; the distance to the bf16 run on the original weights is the
    format's own error and is printed."""
    from test_decode_fp4_gpu import dequantised4
    from test_decode_fp8_gpu import dequantised
    c, cfg, sd, lora, gold = cases[name]
    eq = engine(dev, cfg, sd, lora, BF, training=False, **{"decode_" + form: True})
    assert eq.decode_is_fused(QW.B)
    assert eq.decode_streams_fp8(QW.B) == (form == "fp8") and eq.decode_streams_fp4(QW.B) == (form == "fp4")
    et = engine(dev, cfg, (dequantised if form == "fp8" else dequantised4)(sd), lora, BF, training=False)
    e16 = engine(dev, cfg, sd, lora, BF, training=False)
    # one bf16 prefill on the original weights, shared: the three engines then run the same token steps from the same cache
    x, toks = gold["inputs_embeds"].to(dev, BF), gold["tokens"].to(dev)
    kc, vc = e16.alloc_cache(QW.B, S + STEPS)
    e16.prefill(x, kc, vc)
    caches = {e: (kc.clone(), vc.clone()) for e in (eq, et, e16)}
    for t in range(1, STEPS):
        tok = toks[:, t - 1].contiguous()
        a, b, r = (e.decode_step(tok, S + t - 1, *caches[e]).clone() for e in (eq, et, e16))
        print(f"{name} {form} step {t}: vs bf16 step on dequantised weights {rel_l2(a, b):.3e}; vs bf16 weights {rel_l2(a, r):.3e}; "
              f"vs the fixture {rel_l2(a.cpu(), gold['step_logits'][:, t]):.3e}")
        assert torch.isfinite(a).all()
        assert rel_l2(a, b) < TOKEN_STEP_CODE_FORM_REL_L2, t
        if form == "fp8":
            assert rel_l2(a, r) < Bar.FP8_VS_UNQUANTISED_REL_L2, t
