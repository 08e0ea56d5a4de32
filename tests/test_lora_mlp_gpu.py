"""lora_target_modules: LoRA adapters on gate_proj / up_proj / down_proj (and any subset of the seven modules) on every LLM path, against the
float64 reference of tests/refs64_lora_mlp.py (tied to the pinned oracle by tests/test_lora_targets_cpu.py).

Geometry: Wt.tiny().llama (d 256, ffn 512, 2 layers, V 256), and the same at ffn 320, where down_proj's dropout mask cannot be generated in
the kernels (320 % 256) and the batched gate|up launches do not apply: the materialised-mask and one-launch-per-adapter forms.  Rows: B = 2,
S = 256, or B = 3, S = 40 (M = 120: a row tail in every 16- and 64-row tile).  Bars: tests/bars.py, as every model-level test uses them.
The adapters are strong (refs64_lora_mlp.A_STD, B_STD) so that a missing MLP term is far outside the bars; test_mlp_adapters_matter measures it."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64_lora_mlp as R  # noqa: E402
from bars import rel_l2  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
ALL = R.MODULES
SCALE = 2.0


def _round(sd, dtype):
    return {k: v.to(dtype).float() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _case(ffn, r, targets, dtype, B, S):
    """(config, base weights as the engine of `dtype` holds them, adapters, x, labels): CPU float32 tensors."""
    c, sd = R.tiny_llama(ffn)
    x, labels = R.batch(c, B, S)
    return c, _round(sd, dtype), R.lora_weights(c, r, targets, seed=r), x.to(dtype).float(), labels


def _engine(dev, c, sd, r, targets, lora, dtype, training=True, **kw):
    from avllm.arch import LlamaCfg, LoraCfg
    from avllm.engine import LlamaEngine
    lc = None if targets is None else LoraCfg(r, SCALE * r, tuple(targets))
    return LlamaEngine(sd, LlamaCfg(**vars(c)), lc, lora, dtype=dtype, device=dev, training=training, **kw)


def _masks(dev, eng, c, targets, B, S, p, base=None):
    """The step's masks as the kernels generate them: ops.dropout(ones [M, K], seed_of(l, module), p) at the module's input width K."""
    from avllm import ops
    base = eng.desc.dropout_seed if base is None else base
    out = {}
    for l in range(c.layers):
        for nm in targets:
            K = c.ffn if nm == "down_proj" else c.hidden
            out[f"layers.{l}.{nm}"] = ops.dropout(torch.ones(B * S, K, device=dev, dtype=F32), R.seed_of(base, c.layers, l, nm), p).cpu().view(B, S, K).double()
    return out


def _step(dev, eng, x, labels, dtype, p=0.0, seed=0):
    """One training forward + backward -> (loss, logits, {tensor: grad}, dx_embeds) on the CPU."""
    B, S, d = x.shape
    logits = eng.fwd_loss(x.to(dev).to(dtype), labels.to(dev), want_logits=True, dropout=p, seed=seed)
    eng.lora_g.zero_()
    dx = torch.empty(B, S, d, device=dev, dtype=dtype)
    eng.bwd(dx_embeds=dx)
    loss = float(eng.acc[0] / eng.acc[1])
    return loss, logits.float().cpu(), {k: v.cpu().clone() for k, v in eng.lora_views(eng.lora_g).items()}, dx.float().cpu()


def _check_f32(got, ref):
    loss, logits, grads, dx = got
    rl, rlogits, rg, rdx = ref
    print(f"loss err {abs(loss - float(rl)):.2e}  logits max err {float((logits.double() - rlogits).abs().max()):.2e} (max |ref| {float(rlogits.abs().max()):.2f})")
    assert abs(loss - float(rl)) < Bar.F32_LOSS_ABS
    assert float((logits.double() - rlogits).abs().max()) < Bar.F32_LOGITS_ABS
    assert set(grads) == set(rg)
    for k, ref_t in list(rg.items()) + [("dx_embeds", rdx)]:
        g = dx if k == "dx_embeds" else grads[k]
        e = float((g.double() - ref_t).abs().max()) / float(ref_t.abs().max())
        print(f"  {k}: max err / max |ref| {e:.2e}")
        assert float(ref_t.abs().max()) > 0 and e <= Bar.F32_GRAD_REL_MAX, (k, e)


def _check_bf16(got, ref):
    loss, logits, grads, dx = got
    rl, rlogits, rg, rdx = ref
    keys = sorted(rg)
    allg, allr = torch.cat([grads[k].flatten() for k in keys]), torch.cat([rg[k].flatten() for k in keys])
    print(f"loss err {abs(loss - float(rl)):.2e}  logits rel L2 {rel_l2(logits, rlogits):.2e}  grad rel L2 {rel_l2(allg, allr):.2e}  dx rel L2 {rel_l2(dx, rdx):.2e}")
    assert abs(loss - float(rl)) < Bar.BF16_LOSS_ABS
    assert rel_l2(logits, rlogits) < Bar.BF16_LOGITS_REL_L2
    assert set(grads) == set(rg) and rel_l2(allg, allr) < Bar.BF16_GRAD_REL_L2
    for k in keys:
        print(f"  {k}: rel L2 {rel_l2(grads[k], rg[k]):.2e}")
        assert rel_l2(grads[k], rg[k]) < Bar.BF16_GRAD_TENSOR_REL_L2, (k, rel_l2(grads[k], rg[k]))
    assert rel_l2(dx, rdx) < Bar.BF16_GRAD_TENSOR_REL_L2
    return allg


# ------------------------------------------------------------------------------------------------ 1. fp32, no dropout
@pytest.mark.parametrize("targets,ffn,B,S", [(ALL, 512, 3, 40), (ALL[4:], 512, 2, 256), (("q_proj", "v_proj", "down_proj"), 512, 3, 40), (ALL, 320, 3, 40),
                                              (("k_proj", "gate_proj"), 320, 3, 40)],
                         ids=["all-linear", "mlp-only-S256", "q-v-down", "all-linear-ffn320", "k-gate-ffn320"])
def test_fp32_step(dev, targets, ffn, B, S):
    c, sd, lora, x, labels = _case(ffn, 16, targets, F32, B, S)
    eng = _engine(dev, c, sd, 16, targets, lora, F32)
    assert not eng.decode_is_fused(2) or not eng.mlp_targets
    _check_f32(_step(dev, eng, x, labels, F32), R.step(sd, lora, c, SCALE, x, labels))


# ------------------------------------------------------------------------------------------------ 2. bf16, no dropout
@pytest.mark.parametrize("r,ffn,B,S", [(16, 512, 2, 256), (8, 512, 3, 40), (32, 512, 3, 40), (16, 320, 3, 40)], ids=["r16-S256", "r8", "r32-unbatched", "r16-ffn320"])
def test_bf16_step(dev, r, ffn, B, S):
    c, sd, lora, x, labels = _case(ffn, r, ALL, BF, B, S)
    eng = _engine(dev, c, sd, r, ALL, lora, BF)
    _check_bf16(_step(dev, eng, x, labels, BF), R.step(sd, lora, c, SCALE, x, labels))


# ------------------------------------------------------------------------------------------------ 3. bf16, dropout with the same masks
@pytest.mark.parametrize("ffn,B,S", [(512, 2, 256), (320, 3, 40)], ids=["fused-masks", "ffn320-materialised"])
def test_bf16_dropout_same_masks(dev, ffn, B, S):
    """p = 0.25: the reference is fed the masks the kernels generate -- gate, up at width d, down at width ffn, each from its own seed -- and
    agrees within the bf16 bars; fed masks of another base seed it misses the gradient bar by more than 4 x (the masks are really applied,
    and the same ones in the forward, in dA and in the input gradient)."""
    p, seed = 0.25, 0xBEEF + ffn
    c, sd, lora, x, labels = _case(ffn, 16, ALL, BF, B, S)
    eng = _engine(dev, c, sd, 16, ALL, lora, BF)
    got = _step(dev, eng, x, labels, BF, p=p, seed=seed)
    assert eng.desc.dropout_seed == seed
    masks = _masks(dev, eng, c, ALL, B, S, p)
    assert len({int(m.sum()) for m in masks.values()}) > 1                          # not one mask seven times
    allg = _check_bf16(got, R.step(sd, lora, c, SCALE, x, labels, masks))
    wrong = _masks(dev, eng, c, ALL, B, S, p, base=seed + 1000)
    _, _, og, _ = R.step(sd, lora, c, SCALE, x, labels, wrong)
    miss = rel_l2(allg, torch.cat([og[k].flatten() for k in sorted(og)]))
    print(f"other masks: grad rel L2 {miss:.2e}")
    assert miss > 4 * Bar.BF16_GRAD_REL_L2


# ------------------------------------------------------------------------------------------------ 4. non-vacuity
def test_mlp_adapters_matter(dev):
    c, sd, lora, x, labels = _case(512, 16, ALL, BF, 3, 40)
    eng = _engine(dev, c, sd, 16, ALL, lora, BF)
    _, logits, grads, _ = _step(dev, eng, x, labels, BF)
    zeroed = {k: (torch.zeros_like(v) if k.endswith("lora_B") and k.split(".")[2] in ALL[4:] else v) for k, v in lora.items()}
    _, logits0, _, _ = _step(dev, _engine(dev, c, sd, 16, ALL, zeroed, BF), x, labels, BF)
    moved = rel_l2(logits, logits0)
    print(f"MLP adapters move the logits by {moved:.2e} relative L2")
    assert moved > 4 * Bar.BF16_LOGITS_REL_L2
    for k, g in grads.items():
        if k.split(".")[2] in ALL[4:]:
            assert float(g.abs().max()) > 0, k


# ------------------------------------------------------------------------------------------------ 5. the new kernel
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,f", [(1, 64), (120, 64), (1, 320), (120, 320)])
def test_swiglu_bwd_h(dev, dtype, M, f):
    """dgu as swiglu_bwd's bar has it; h = silu(g) * u within silu_bar(g) |u| plus one product rounding (plus the bf16 output rounding); and
    both equal, bit for bit, what the two kernels it stands in for write."""
    from avllm import ops
    from oracle import weights as Wt
    gu = (Wt._randn("sw.gu", M + f, (M, 2 * f), 2.0)).to(dtype).to(dev)
    dh = (Wt._randn("sw.dh", M + f, (M, f), 1.0)).to(dtype).to(dev)
    dgu, h = ops.swiglu_bwd_h(dh, gu)
    g, u, d64 = gu[:, :f].double().cpu(), gu[:, f:].double().cpu(), dh.double().cpu()
    s = torch.sigmoid(g)
    ref_h = g * s * u
    ref_dgu = torch.cat([d64 * u * (s * (1 + g * (1 - s))), d64 * g * s], 1)
    bar_h = Bar.silu_bar(g) * u.abs() + Bar.U32 * ref_h.abs() + Bar.FP32_DENORM
    bar_d = Bar.swiglu_bwd_bar(d64, g, u)
    if dtype == BF:
        bar_h, bar_d = bar_h + Bar.BF16_OUT_REL * ref_h.abs(), bar_d + Bar.BF16_OUT_REL * ref_dgu.abs()
    eh, ed = (h.double().cpu() - ref_h).abs(), (dgu.double().cpu() - ref_dgu).abs()
    print(f"h worst err / bar {float((eh / bar_h).max()):.3f}, dgu worst err / bar {float((ed / bar_d).max()):.3f}")
    assert bool((eh <= bar_h).all()) and bool((ed <= bar_d).all())
    assert torch.equal(dgu, ops.swiglu_bwd(dh, gu)) and torch.equal(h, ops.swiglu_fwd(gu))
    with pytest.raises(ValueError):
        ops.swiglu_bwd_h(dh[:, :-4].contiguous(), gu)


# ------------------------------------------------------------------------------------------------ 6. the default is unchanged
def _tiny_model(dev, W=None, **kw):
    import kv8_cases as K
    from avllm.arch import ClipCfg, LlamaCfg, LoraCfg, ModelCfg, WhisperCfg
    from avllm.model import ClipWhisperModel
    oc, W0, _, _ = K.tiny()
    cfg = ModelCfg(WhisperCfg(**vars(oc.whisper)), ClipCfg(**vars(oc.clip)), LlamaCfg(**vars(oc.llama)), LoraCfg(oc.lora.r, oc.lora.alpha))
    kw.setdefault("precision", "bf16")
    kw.setdefault("lora_dropout", 0.0)
    return ClipWhisperModel(device="cuda:0", lora_r=oc.lora.r, lora_alpha=oc.lora.alpha, max_seq_len=256, config=cfg,
                            weights=W0 if W is None else W, **kw)


def _tiny_batch():
    import kv8_cases as K
    from oracle import weights as Wt
    oc, _, frames, batch_seed = K.tiny()
    audio, video, labels, prompt = Wt.synthetic_batch(oc, 2, frames, seed=batch_seed)
    return audio, video, labels[:, :64].contiguous(), prompt


def test_default_targets_unchanged(dev):
    """No keyword, None, and the four names spelled out are one model: the layout (per_layer, views, slices), logits, lora_g and
    state_dict() bit for bit, under dropout (the seeds of q, k, v, o are what they were).  The loss is the one output that two runs of ONE
    model do not repeat bit for bit: avllm_ce_fwd adds the scored rows' terms to loss_sum with float atomics, in whatever order the rows
    finish (so it was before the keyword; seen here as 5.8074 twice with different last bits).  Its addends are functions of the logits,
    which are compared bit for bit; the sum is held to the bound of re-ordering n positive fp32 addends, n * 2^-24 relative.  M = 128 rows:
    every gradient reduction over tokens is one chunk, so lora_g has one adder per element and does repeat."""
    audio, video, labels, prompt = _tiny_batch()
    outs = []
    for kw in ({}, {"lora_target_modules": None}, {"lora_target_modules": ["o_proj", "q_proj", "v_proj", "k_proj"]}):
        m = _tiny_model(dev, lora_dropout=0.1, **kw).train()
        eng = m.llm_engine
        out = m(audio=audio.to(dev), video=video.to(dev), prompt=prompt.to(dev), labels=labels.to(dev))
        out["loss"].backward()
        r, d = eng.r, eng.cfg.hidden
        assert eng.per_layer == 4 * r * 2 * d and m.lora_target_modules == ALL[:4] and eng._slices(1, 3) == eng._slices(1, "o_proj")
        assert eng._slices(1, 2) == ((eng.per_layer + 4 * r * d, eng.per_layer + 5 * r * d), (eng.per_layer + 5 * r * d, eng.per_layer + 6 * r * d))
        assert list(eng.lora_views()) == [f"layers.{i}.{nm}.lora_{ab}" for i in range(2) for nm in ALL[:4] for ab in "AB"]
        assert eng._pack_table.shape == (8, 8) and eng._pack_table_f is None
        assert all(not ly.lora_mlp[k].A_pad for ly in eng.layers for k in range(3)) and eng.decode_is_fused(2)
        outs.append((out["loss"].detach().clone(), out["logits"].clone(), eng.lora_g.clone(), m.state_dict()))
    for o in outs[1:]:
        n_scored = int((labels[:, 1:] != 2).sum())                                  # pad_token_id 2 -> -100; an upper bound is all that is needed
        assert abs(float(o[0]) - float(outs[0][0])) <= max(n_scored, 1) * Bar.U32 * float(outs[0][0]), (float(o[0]), float(outs[0][0]))
        assert torch.equal(o[1], outs[0][1]), "logits"
        assert torch.equal(o[2], outs[0][2]), "lora_g"
        assert list(o[3]) == list(outs[0][3]) and all(torch.equal(o[3][k], outs[0][3][k]) for k in o[3])
    assert float(outs[0][2].abs().max()) > 0 and all(".self_attn." in k for k in outs[0][3] if "lora_" in k)


def test_refusals(dev):
    with pytest.raises(ValueError, match="use_lora=False"):
        _tiny_model(dev, use_lora=False, lora_target_modules="all-linear")
    with pytest.raises(ValueError, match="fc1"):
        _tiny_model(dev, lora_target_modules="q_proj,fc1")
    with pytest.raises(ValueError, match="empty"):
        _tiny_model(dev, lora_target_modules=[])
    with pytest.raises(ValueError, match="duplicate module 'up_proj'"):
        _tiny_model(dev, lora_target_modules=["up_proj", "up_proj"])
    with pytest.raises(NotImplementedError, match="down_proj"):
        _tiny_model(dev, precision="fp8", lora_target_modules="q_proj,down_proj")
    c, sd, lora, _, _ = _case(512, 16, ALL, BF, 3, 40)
    with pytest.raises(NotImplementedError, match="gate_proj"):
        _engine(dev, c, sd, 16, ("gate_proj",), None, BF, fp8=True)


# ------------------------------------------------------------------------------------------------ 7. eval forward and greedy generate, unmerged
N_NEW = 12


def _greedy(dev, eng, x, vocab, n):
    from avllm import generation
    procs = generation.LogitsProcessors(vocab=vocab, eos=None, device=dev, max_new_tokens=n)
    return generation.token_loop(eng, x.to(dev).to(BF), None, 0, n, procs).cpu()


def _held(ids, ref, margins, thr):
    """Where the reference's top-2 margin exceeds thr the token is the reference's; at a near-tie either, and the row ends there if they part."""
    held = 0
    for b in range(ref.shape[0]):
        for t in range(ref.shape[1]):
            same = int(ids[b, t]) == int(ref[b, t])
            if float(margins[b, t]) > thr:
                assert same, (b, t, ids[b].tolist(), ref[b].tolist(), margins[b].tolist())
                held += 1
            elif not same:
                break
    return held


@pytest.mark.parametrize("targets", [ALL, ("q_proj", "up_proj", "down_proj")], ids=["all-linear", "q-up-down"])
def test_eval_forward_and_greedy_unmerged(dev, targets):
    """Prefill logits of every position and the general token step with the adapters attached, against float64; the step is the general
    one (an unmerged MLP adapter leaves the fused path), with every flag that goes with the fused path off."""
    c, sd, lora, x, _ = _case(512, 16, targets, BF, 3, 40)
    eng = _engine(dev, c, sd, 16, targets, lora, BF, training=False, decode_fp8=True, kv_fp8=True)
    assert not eng.decode_is_fused(3) and not eng.decode_streams_fp8(3) and not eng.decode_streams_fp4(3)
    assert not eng.decode_caches_fp8(3) and not eng.decode_shares_prefix(3)
    kc, vc = eng.alloc_cache(3, 40)
    assert kc.dtype == BF
    _, full = eng.prefill(x.to(dev).to(BF), kc, vc, all_logits=True)
    ref = R.logits64(sd, lora, c, SCALE, x)
    e = rel_l2(full.float().cpu(), ref)
    print(f"prefill logits rel L2 {e:.2e}")
    assert e < Bar.BF16_LOGITS_REL_L2
    with eng.adapters_disabled():                                                  # all seven modules off: the frozen model
        _, bare = eng.prefill(x.to(dev).to(BF), kc, vc, all_logits=True)
    assert rel_l2(bare.float().cpu(), R.logits64(sd, None, c, SCALE, x)) < Bar.BF16_LOGITS_REL_L2 and rel_l2(bare.float().cpu(), ref) > 4 * Bar.BF16_LOGITS_REL_L2
    ids = _greedy(dev, eng, x, c.vocab, N_NEW)
    rid, margins = R.greedy(sd, lora, c, SCALE, x, N_NEW)
    thr = 2.0 * Bar.BF16_LOGIT_MAX_ABS * max(1.0, float(ref.abs().max()))
    held = _held(ids, rid, margins, thr)
    print(f"greedy: {held} of {rid.numel()} decisions held at margin > {thr:.3f}")
    assert int((margins > thr).sum()) >= 8 and held >= 1                            # 8 or 9 of the 36 decisions are clear ones (measured on the CPU)


# ------------------------------------------------------------------------------------------------ 8. merge_lora()
@pytest.mark.parametrize("form", ["bf16", "fp8", "fp4"])
def test_merge_lora(dev, form):
    import refs64_merge as M
    from bars_merge import merge_bar
    kw = {"fp8": dict(decode_fp8=True), "fp4": dict(decode_fp4=True), "bf16": {}}[form]
    c, sd, lora, x, _ = _case(512, 16, ALL, BF, 3, 40)
    eng = _engine(dev, c, sd, 16, ALL, lora, BF, training=True, **kw)
    assert not eng.decode_is_fused(2)
    eng.merge_lora()
    out = eng.merged_llm_state_dict()
    for i in range(c.layers):
        for nm in ALL:
            key = f"model.layers.{i}.{'mlp' if nm in ALL[4:] else 'self_attn'}.{nm}.weight"
            ref, u, sum_abs = M.merge64(sd[key], lora[f"layers.{i}.{nm}.lora_A"], lora[f"layers.{i}.{nm}.lora_B"], SCALE)
            ratio = float(((out[key].double().cpu() - ref).abs() / merge_bar(ref, u, sum_abs, 16, SCALE, True)).max())
            assert ratio <= 1.0 and not torch.equal(out[key].float().cpu(), sd[key]), (key, ratio)
    assert all(not lm.A_pad and not lm.B_pad for ly in eng.layers for lm in list(ly.lora) + list(ly.lora_mlp))
    assert all(not ly.wgu_t and not ly.wdown_t and not ly.wqkv_t and not ly.wo_t for ly in eng.layers), "the stale transposed copies are gone"
    assert eng.decode_is_fused(2) and eng.decode_streams_fp8(2) == (form == "fp8") and eng.decode_streams_fp4(2) == (form == "fp4")
    plain = _engine(dev, c, {k: v.float().cpu() for k, v in out.items()}, 16, None, None, BF, training=False, **kw)
    assert plain.decode_is_fused(2)
    xb = x[:2]
    a, b = _greedy(dev, eng, xb, c.vocab, N_NEW), _greedy(dev, plain, xb, c.vocab, N_NEW)
    assert torch.equal(a, b), (form, a.tolist(), b.tolist())                        # same kernels on the same bytes: the images were rebuilt
    fulls = []
    for e_ in (eng, plain):
        kc, vc = e_.alloc_cache(2, 40, fp8=False)
        fulls.append(e_.prefill(xb.to(dev).to(BF), kc, vc, all_logits=True)[1])
    assert torch.equal(fulls[0], fulls[1])
    assert rel_l2(fulls[0].float().cpu(), R.logits64(sd, lora, c, SCALE, xb)) < Bar.BF16_LOGITS_REL_L2
    with pytest.raises(RuntimeError, match="merge_lora"):
        eng.fwd_loss(x.to(dev).to(BF), torch.zeros(3, 40, dtype=torch.long, device=dev))


# ------------------------------------------------------------------------------------------------ 9. the model's surfaces and the trainer
def _all_linear_weights():
    import kv8_cases as K
    oc, W0, _, _ = K.tiny()
    W = dict(W0)
    W["lora"] = R.lora_weights(oc.llama, oc.lora.r, ALL, seed=9, a_std=0.01 / oc.lora.r, b_std=0.05)
    return oc, W


def test_model_keys_and_pretrained_round_trip(dev, tmp_path):
    oc, W = _all_linear_weights()
    m = _tiny_model(dev, W, lora_target_modules="all-linear")
    assert m.lora_target_modules == ALL and m.llm_engine.targets == ALL
    sd = m.state_dict()
    d, f, r = oc.llama.hidden, oc.llama.ffn, oc.lora.r
    P = "llm.base_model.model.model.layers.1.mlp."
    assert sd[P + "gate_proj.lora_A.default.weight"].shape == (r, d) and sd[P + "gate_proj.lora_B.default.weight"].shape == (f, r)
    assert sd[P + "up_proj.lora_A.default.weight"].shape == (r, d) and sd[P + "up_proj.lora_B.default.weight"].shape == (f, r)
    assert sd[P + "down_proj.lora_A.default.weight"].shape == (r, f) and sd[P + "down_proj.lora_B.default.weight"].shape == (d, r)
    assert torch.equal(sd[P + "down_proj.lora_A.default.weight"].cpu(), W["lora"]["layers.1.down_proj.lora_A"])
    assert sum("lora_" in k for k in sd) == 2 * 7 * 2
    m.save_pretrained(str(tmp_path / "saved"))
    from avllm.model import ClipWhisperModel
    W2 = {k: v for k, v in W.items() if k != "lora"}
    m2 = ClipWhisperModel.from_pretrained(str(tmp_path / "saved"), device="cuda:0", config=m.cfg, weights=W2, precision="bf16", lora_dropout=0.0)
    assert m2.lora_target_modules == ALL and torch.equal(m2.llm_engine.lora_p, m.llm_engine.lora_p)
    # synthetic adapters of a model that is given none: the reference's init on all seven
    v = m2.llm_engine.lora_views(_tiny_model(dev, W2, lora_target_modules="all-linear", seed=4).llm_engine.lora_p)
    assert float(v["layers.0.up_proj.lora_A"].abs().max()) > 0 and float(v["layers.0.up_proj.lora_B"].abs().max()) == 0
    # a LoRA tensor of a module the model does not adapt is refused by name, not dropped
    plain = _tiny_model(dev, W2)
    key = P + "down_proj.lora_A.default.weight"
    with pytest.raises(ValueError, match="layers.1.mlp.down_proj.lora_A"):
        plain.load_state_dict({key: sd[key]})
    with pytest.raises(KeyError, match="layers.1.down_proj.lora_A"):
        plain.llm_engine.load_lora({"layers.1.down_proj.lora_A": sd[key]})


def test_trainer_steps_and_resume(dev, tmp_path):
    from avllm.trainer import ClipWhisperTrainer
    oc, W = _all_linear_weights()
    audio, video, labels, prompt = _tiny_batch()
    m = _tiny_model(dev, W, lora_target_modules="all-linear", precision="fp32").train()
    tr = ClipWhisperTrainer(m, learning_rate=1e-3, grad_clip=0.5, total_steps=10, max_epochs=1, output_dir=str(tmp_path), use_graph=False)
    assert tr._lora_keys() == [k for k in m.state_dict() if "lora_" in k]
    before = {k: v.clone() for k, v in m.llm_engine.lora_views().items()}
    for _ in range(2):
        tr.train_step(audio.to(dev), video.to(dev), labels.to(dev), prompt.to(dev))
    after = m.llm_engine.lora_views()
    for k in before:
        if k.split(".")[2] in ALL[4:]:
            assert not torch.equal(before[k], after[k]), f"{k} did not move"
    tr._save_checkpoint(0, "ck.pt")
    path = str(tmp_path / "ck.pt")
    assert ClipWhisperTrainer.checkpoint_lora_targets(path) == list(ALL)
    W2 = {k: v for k, v in W.items() if k != "lora"}
    m2 = _tiny_model(dev, W2, lora_target_modules=ClipWhisperTrainer.checkpoint_lora_targets(path), precision="fp32", seed=3).train()
    assert not torch.equal(m2.llm_engine.lora_p, m.llm_engine.lora_p)
    tr2 = ClipWhisperTrainer(m2, learning_rate=1e-3, grad_clip=0.5, total_steps=10, max_epochs=1, output_dir=str(tmp_path), use_graph=False)
    tr2.load_checkpoint(path)
    assert m2.lora_target_modules == ALL and torch.equal(m2.llm_engine.lora_p, m.llm_engine.lora_p)
    assert tr2.global_step == 2 and torch.equal(tr2.m, tr.m) and torch.equal(tr2.v, tr.v)
    with pytest.raises(ValueError, match="lora_target_modules"):
        ClipWhisperTrainer(_tiny_model(dev, W2, precision="fp32").train(), learning_rate=1e-3, total_steps=10, max_epochs=1, output_dir=str(tmp_path),
                           use_graph=False).load_checkpoint(path)
