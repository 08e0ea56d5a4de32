"""tests/train_step_cases.py and the extended tests/refs64_lora_mlp.py checked on the CPU before tests/test_train_step_matrix_gpu.py leans on them:

  * coverage: the case list holds every pair of levels of every two factors but the refused ones, the two named deployments, at most 24 entries,
    and every launch form of forms() is seen taken and not taken;
  * the reference is tied down: with its defaults it is the arithmetic it was (a copy of the former decoder is kept here for that), with
    biases and head norms it reproduces transformers' logits, loss, adapter gradients and d loss / d inputs_embeds of the g12 and g13 fixtures,
    and in fp8 form its hook is oracle.avsr_oracle._LinearFp8 product by product and its logits are those of the oracle's decoder under
    fp8_mode(encoders=False) on the rows no flipped e4m3 decision reached (the test says why some are).  (The control against
    oracle.avsr_oracle.train_step_grads on the default targets stays where it was: tests/test_lora_targets_cpu.py.);
  * headroom: for every bf16 case the forward with every stored activation rounded to bf16 stays within HALF of BF16_LOGITS_REL_L2 of the float64
    logits (a case that had not would get another seed, never another bar).  Gradients have no rounded restatement on the host: their headroom
    is what the MI355X run measures, recorded in DESIGN.md;
  * sensitivity: the reference with one planted defect, judged by train_step_cases.ratios -- the function the GPU test asserts with -- misses
    the case's bars by more than 10 x on some case that carries the feature and by more than 2 x on EVERY fp32 or bf16 case that carries it; the
    fp8 carriers' ratios are printed.

Dropout masks here are host-drawn Bernoulli masks (train_step_cases.host_masks); the GPU test feeds the reference the kernels' own."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_bias_weights as AW
import qwen3_weights as QW
import refs64_kv8 as R8
import refs64_lora_mlp as R
import train_step_cases as TC
from bars import BF16_LOGITS_REL_L2, F32_GRAD_REL_MAX, F32_LOGITS_ABS, F32_LOSS_ABS, rel_l2

_BASE = {}


def base(c):
    """Per case, computed once and left unchanged: (host masks or None, the float64 step with them)."""
    if c.name not in _BASE:
        masks = TC.host_masks(c)
        _BASE[c.name] = (masks, TC.ref_step(c, masks))
    return _BASE[c.name]


# ---------------------------------------------------------------- coverage
def test_the_case_list_covers_every_pair_of_levels():
    assert len(TC.CASES) <= 24 and len({c.name for c in TC.CASES}) == len(TC.CASES)
    for c in TC.CASES:
        assert all(getattr(c, f) in lv for f, lv in TC.FACTORS.items()), c.id
        assert not any(getattr(c, fa) == a and getattr(c, fb) == b for fa, a, fb, b in TC.IMPOSSIBLE), c.id
    assert TC.missing_pairs() == []
    a, q = TC.CASES[0], TC.CASES[1]
    assert a.name == "default-deployment" and (a.geom, a.precision, a.modules, a.rank, a.norms, a.bias) == ("g512", "bf16", R.MODULES[:4], 16, 0, "none") and a.p > 0
    assert q.name == "qwen3-all-linear" and (q.norms, q.theta, q.modules) == (1, 1e6, R.MODULES)
    # the check itself can fail: of an empty list every possible pair is missing, of the two deployments alone all but their 45 each
    n = [len(lv) for lv in TC.FACTORS.values()]
    total = (sum(n) ** 2 - sum(k * k for k in n)) // 2 - len(TC.IMPOSSIBLE)
    assert len(TC.missing_pairs([])) == total and total - 90 <= len(TC.missing_pairs(TC.CASES[:2])) < total - 45
    assert all(p in TC.missing_pairs([]) or p in TC.IMPOSSIBLE for p in [("precision", "fp8", "targets", "all"), ("geom", "g896", "precision", "fp8")])
    for c in TC.CASES:
        x, labels = TC.inputs(c)
        scored = (labels != -100).any(1)
        assert x.shape == (c.B, c.S, c.hidden) and torch.equal(x, x.to(TC.engine_dtype(c)).float())
        assert scored.tolist() == ([True, False, True] if c.rows == "3x40" else [True] * c.B), c.id
        base_seed, host, devw = TC.seeds(c)
        assert (host + (devw or 0)) & 0xFFFFFFFF == base_seed and (devw is not None) == (c.drop == "dev") and (devw is None or host != base_seed)


def test_every_launch_form_is_seen_taken_and_not_taken():
    seen = {}
    for c in TC.CASES:
        for k, v in TC.forms(c).items():
            seen.setdefault(k, set()).add(bool(v))
    assert set(seen) == {"fwd_qkv_batch", "bwd_qkv_batch", "fwd_gu_batch", "bwd_gu_batch", "mask_fused_d", "mask_fused_f", "seg_qkv", "seg_o", "seg_gu",
                         "seg_down", "rope_fused"}
    assert all(v == {True, False} for v in seen.values()), {k: v for k, v in seen.items() if v != {True, False}}
    f = {c.name: TC.forms(c) for c in TC.CASES}
    # the crossings the geometries were chosen for: g512n batches the forward but not the backward and fuses the mask at d but not at ffn; an
    # fp8 case batches the backward it could not batch forward; g896 batches and fuses nothing
    pair = lambda a, b: {(v[a], v[b]) for v in f.values()}      # noqa: E731
    assert (True, False) in pair("fwd_qkv_batch", "bwd_qkv_batch") and (False, True) in pair("fwd_qkv_batch", "bwd_qkv_batch")
    assert (True, False) in pair("fwd_gu_batch", "bwd_gu_batch") and (True, True) in pair("fwd_gu_batch", "bwd_gu_batch")
    down_dropped = [TC.forms(c) for c in TC.CASES if c.p > 0 and "down_proj" in c.modules]
    assert {(v["mask_fused_d"], v["mask_fused_f"]) for v in down_dropped} >= {(True, True), (True, False), (False, False)}
    assert not any(v for c in TC.CASES if c.geom == "g896" for k, v in TC.forms(c).items() if "batch" in k or "mask" in k)
    # what cannot vary here (the module docstring of train_step_cases says why)
    assert all(TC.forms(c)["rope_fused"] == (c.precision != "fp32") for c in TC.CASES)


# ---------------------------------------------------------------- the reference is tied down
def _hidden_before(sd, lora, c, scale, x, masks=None):
    """refs64_lora_mlp.hidden as it was before biases, head norms, the "llama3" rule, proj, rnd and wrong were added: kept to compare against."""
    def adapted(x, w, key):
        y = x @ w.T
        if lora is not None and key + ".lora_A" in lora:
            xl = x * masks[key].to(x.dtype).view_as(x) if masks is not None and key in masks else x
            y = y + scale * ((xl @ lora[key + ".lora_A"].T) @ lora[key + ".lora_B"].T)
        return y
    B, T, d = x.shape
    H, hd = c.heads, c.head_dim
    Hkv = getattr(c, "kv_heads", 0) or H
    cos, sin = R.rope_table(0, T, hd, c.theta)
    for i in range(c.layers):
        P, K = f"model.layers.{i}.", f"layers.{i}."
        h = R.rms_norm(x, sd[P + "input_layernorm.weight"], c.eps)
        sp = lambda t, n: t.view(B, T, n, hd).transpose(1, 2)      # noqa: E731
        q = R.rope(sp(adapted(h, sd[P + "self_attn.q_proj.weight"], K + "q_proj"), H), cos, sin)
        k = R.rope(sp(adapted(h, sd[P + "self_attn.k_proj.weight"], K + "k_proj"), Hkv), cos, sin)
        v = sp(adapted(h, sd[P + "self_attn.v_proj.weight"], K + "v_proj"), Hkv)
        if Hkv != H:
            k, v = k.repeat_interleave(H // Hkv, dim=1), v.repeat_interleave(H // Hkv, dim=1)
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        s = s.masked_fill(~torch.ones(T, T, dtype=torch.bool).tril(), float("-inf"))
        a = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, d)
        x = x + adapted(a, sd[P + "self_attn.o_proj.weight"], K + "o_proj")
        h = R.rms_norm(x, sd[P + "post_attention_layernorm.weight"], c.eps)
        g = adapted(h, sd[P + "mlp.gate_proj.weight"], K + "gate_proj")
        u = adapted(h, sd[P + "mlp.up_proj.weight"], K + "up_proj")
        x = x + adapted(g * torch.sigmoid(g) * u, sd[P + "mlp.down_proj.weight"], K + "down_proj")
    return R.rms_norm(x, sd["model.norm.weight"], c.eps)


def test_defaults_leave_the_reference_as_it_was():
    """No bias or norm keys, no rope_scaling, proj / rnd / wrong at their defaults: hidden() is bit for bit the former decoder, on the model of
    tests/test_lora_mlp_gpu.py with all seven adapters under masks and on a grouped-query case of this table; step()'s loss, logits, gradients
    and d loss / d x are bit for bit what autograd gives through the former decoder."""
    c, sd = R.tiny_llama(320)
    lora = R.lora_weights(c, 16, R.MODULES, seed=16)
    x, labels = R.batch(c, 3, 40)
    g = torch.Generator().manual_seed(3)
    masks = {f"layers.{l}.{nm}": (torch.rand(3, 40, c.ffn if nm == "down_proj" else c.hidden, generator=g) > 0.25).double() / 0.75
             for l in range(c.layers) for nm in R.MODULES}
    cg = TC.BY_NAME["c18"]
    sdg, lorag = TC.weights(cg)
    xg, labg = TC.inputs(cg)
    for c_, sd_, lora_, x_, lab_, m_ in ((c, sd, lora, x, labels, masks), (c, sd, lora, x, labels, None), (cg, sdg, lorag, xg[:, :48], labg[:, :48], None)):
        sd64, lo64 = R.to64(sd_), R.to64(lora_)
        with torch.no_grad():
            assert torch.equal(R.hidden(sd64, lo64, c_, 2.0, x_.double(), m_), _hidden_before(sd64, lo64, c_, 2.0, x_.double(), m_))
            assert torch.equal(R.hidden(sd64, lo64, c_, 2.0, x_.double(), m_, None, 0, None, None, ()), _hidden_before(sd64, lo64, c_, 2.0, x_.double(), m_))
        loss, logits, grads, dx = R.step(sd_, lora_, c_, 2.0, x_, lab_, m_)
        xr = x_.double().clone().requires_grad_(True)
        lr = {k: v.double().clone().requires_grad_(True) for k, v in lora_.items()}
        lg = _hidden_before(sd64, lr, c_, 2.0, xr, m_) @ sd64["lm_head.weight"].T
        ls = R.shifted_ce(lg, lab_)
        ls.backward()
        assert torch.equal(loss, ls.detach()) and torch.equal(logits, lg.detach()) and torch.equal(dx, xr.grad)
        assert set(grads) == set(lr) and all(torch.equal(grads[k], lr[k].grad) for k in lr)


@pytest.mark.parametrize("family,name", [("g12", "q"), ("g12", "l"), ("g13", "a"), ("g13", "b")])
def test_reference_reproduces_the_transformers_fixtures(golden_dir, family, name):
    """Biases on q, k, v (g12 q) and o as well (g12 l), head norms (g13), query groups of 2 and 7, adapters on: step() against what transformers
    wrote -- logits, loss, every grad.* tensor and dx_embeds -- at the fp32 bars; and the term under test is what ties it."""
    mod = AW if family == "g12" else QW
    c = mod.CASES[name]
    z = np.load(os.path.join(golden_dir, mod.golden_name(c)))
    gold = {k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files}
    sd, lora = mod.weights(c)
    scale = mod.ALPHA / mod.RANK
    x, labels = gold["inputs_embeds"], gold["labels"]
    loss, logits, grads, dx = R.step(sd, lora, c, scale, x, labels)
    rel_max = lambda a, b: float((a - b.double()).abs().max()) / float(b.abs().max())      # noqa: E731
    e_logits, e_loss = float((logits - gold["logits"].double()).abs().max()), abs(float(loss) - float(gold["loss"]))
    e_grad = {k: rel_max(g, gold["grad." + k]) for k, g in grads.items()}
    e_dx = rel_max(dx, gold["dx_embeds"])
    print(f"{family} {name}: |logits| {e_logits:.2e}  |loss| {e_loss:.2e}  worst grad tensor {max(e_grad.values()):.2e}  dx_embeds {e_dx:.2e} (relative to max |ref|)")
    assert {"grad." + k for k in grads} == {k for k in gold if k.startswith("grad.")}
    assert e_logits < F32_LOGITS_ABS and e_loss < F32_LOSS_ABS
    assert max(e_grad.values()) <= F32_GRAD_REL_MAX and e_dx <= F32_GRAD_REL_MAX
    other = AW.without_biases(sd) if family == "g12" else QW.with_swapped_norms(sd)
    _, lo, go, _ = R.step(other, lora, c, scale, x, labels)
    assert float((lo - gold["logits"].double()).abs().max()) > 100 * F32_LOGITS_ABS
    assert max(rel_max(go[k], gold["grad." + k]) for k in go) > 100 * F32_GRAD_REL_MAX


def test_fp8_form_is_the_oracles_fp8_mode():
    """The reference with proj = fp8_proj against oracle.avsr_oracle.llama_hidden / _proj_llm / causal_lm_loss under fp8_mode(encoders=False), on
    the first fp8 case of the table with rows 3x40, without its biases and norms (the oracle has neither; it runs in float32): q|k|v, o, gate|up, down and
    lm_head quantised, the adapter terms not, the backward straight through.  The agreement is measured and printed.  Held to the fp32 bars:
    (a) the hook against the oracle's _LinearFp8 product by product, forward and backward, and (b) the logits rows of the oracle's own
    decoder that no flipped quantisation decision reached (see below for why some are).  Without the hook the comparison misses by far."""
    from oracle import avsr_oracle as O
    c0 = next(c for c in TC.CASES if c.precision == "fp8" and c.rows == "3x40")      # three short sequences: a flip (below) stays in its own
    c = TC.variant(c0, norms=0, bias="none")
    sd, lora = TC.weights(c)
    x, labels = TC.inputs(c)
    masks = TC.host_masks(c)
    got = TC.ref_step(c, masks)
    lo = {k: v.clone().requires_grad_(True) for k, v in lora.items()}
    xo = x.clone().requires_grad_(True)
    masks32 = None if masks is None else {k: v.float() for k, v in masks.items()}
    with O.fp8_mode(encoders=False):
        h = O.llama_hidden(sd, lo, c, SimpleNamespace(scale=c.scale), xo, masks=masks32)
        logits = O._proj_llm(h, sd["lm_head.weight"])
        loss = O.causal_lm_loss(logits, labels)
        loss.backward()
    want = (loss.detach().double(), logits.detach().double(), {k: v.grad for k, v in lo.items()}, xo.grad)
    f32 = TC.without(c, precision="fp32")                            # judged at the fp32 bars
    # (a) the rule, product by product on the case's own matrices: the hook against the oracle's _LinearFp8 on the same input.  Every e4m3
    # decision is then the same and what is left is the oracle's fp32 summation, bounded in any order by K 2^-24 sum |a| |w| on the quantised
    # operands; the backward is dy W on the unquantised weights in both
    from bars import U32
    from oracle import mxfp8
    g = torch.Generator().manual_seed(c.seed)
    for key in ("model.layers.0.self_attn.q_proj.weight", "model.layers.1.self_attn.o_proj.weight", "model.layers.0.mlp.up_proj.weight",
                "model.layers.1.mlp.down_proj.weight", "lm_head.weight"):
        w = sd[key]
        a64 = (torch.randn(40, w.shape[1], generator=g, dtype=torch.float64) * 0.7).requires_grad_(True)
        a32 = a64.detach().float().requires_grad_(True)
        dy = torch.randn(40, w.shape[0], generator=g, dtype=torch.float64)
        y64, y32 = R.fp8_proj(a64, w.double()), O._LinearFp8.apply(a32, w)
        y64.backward(dy)
        y32.backward(dy.float())
        fq = lambda t: mxfp8.fake_quant(t.to(torch.bfloat16).float()).double().abs()      # noqa: E731
        bound = w.shape[1] * U32 * (fq(a32.detach()) @ fq(w).T)
        worst_fwd = float(((y64.detach() - y32.detach().double()).abs() / bound).max())
        print(f"FP8 RULE {key}: hook vs oracle._LinearFp8, worst |difference| / fp32 summation bound {worst_fwd:.3f}")
        assert worst_fwd <= 1.0 and float(y64.detach().abs().max()) > 0
        assert torch.equal(a64.grad, dy @ w.double()) and float((a64.grad - a32.grad.double()).abs().max()) <= 1e-5 * float(a64.grad.abs().max())
    # (b) the placement: the oracle's own decoder in float32.  Its activations differ from the float64 ones in the last fp32 bits, so of the
    # ~10^6 elements that pass a quantiser some round to the other bf16 neighbour and take another e4m3 code: each such flip moves its own
    # row and the later rows of its sequence by up to 1e-1, and the gradients, sums over rows, with them.  Which rows depends on the host's
    # fp32 summation order, so no share of the tensor is promised beyond the first positions of the three sequences: the best tenth of the
    # rows must agree to a tenth of the fp32 logits bar (an error of the hook's placement is in every row: of the unquantised reference no
    # row is within the bar).  The loss and gradient figures are printed; the gradients must be nearer the oracle than the unquantised
    # reference's are, and the backward rule itself is tied exactly in (a)
    r = TC.ratios(f32, got, want)
    plain = TC.ratios(f32, R.step(sd, lora, c, c.scale, x, labels, masks), want)
    row_err = (got[1] - want[1]).abs().amax(-1).flatten()
    row_plain = (R.logits64(sd, lora, c, c.scale, x, masks) - want[1]).abs().amax(-1).flatten()
    clean = float((row_err < F32_LOGITS_ABS).double().mean())
    print(f"FP8 RULE {c.id}: vs the oracle's fp8 mode, error / fp32 bar: {TC.show(r)}; rows within the logits bar {clean:.3f}, median row error "
          f"{float(row_err.median()):.2e}")
    print(f"FP8 RULE {c.id}: the unquantised reference vs the same: {TC.show(plain)}; rows within the logits bar "
          f"{float((row_plain < F32_LOGITS_ABS).double().mean()):.3f}")
    best_tenth = float(row_err.kthvalue(max(1, row_err.numel() // 10)).values)
    assert best_tenth < 0.1 * F32_LOGITS_ABS and float(row_plain.min()) > F32_LOGITS_ABS, (best_tenth, float(row_plain.min()))
    assert plain["tensor"] > r["tensor"] and plain["dx_embeds"] > r["dx_embeds"], (r, plain)


# ---------------------------------------------------------------- headroom
@pytest.mark.parametrize("c", [c for c in TC.CASES if c.precision == "bf16"], ids=lambda c: c.id)
def test_bf16_roundings_leave_half_the_bar(c):
    """The forward with a bf16 rounding wherever the engine stores a tensor (the normed inputs, q|k|v after the bias, q and k after norm and
    RoPE, the attention output, the rank-side products, both residual sums, gate|up, the SwiGLU product, the final norm, the logits)."""
    masks, (_, want, _, _) = base(c)
    sd, lora = TC.weights(c)
    x, _ = TC.inputs(c)
    got = R8.round_bf16(R.logits64(sd, lora, c, c.scale, x, masks, rnd=R8.round_bf16))
    e = rel_l2(got, want)
    print(f"HEADROOM {c.id}: bf16-rounded forward vs float64, logits relative L2 {e:.2e} = {e / BF16_LOGITS_REL_L2:.3f} of the bar")
    assert e < 0.5 * BF16_LOGITS_REL_L2


# ---------------------------------------------------------------- sensitivity
def _first(c, *names):
    return next(nm for nm in names if nm in c.modules)


def _swap_gate_up_B(lora):
    out = dict(lora)
    for k in lora:
        if k.endswith("gate_proj.lora_B"):
            up = k.replace("gate_proj", "up_proj")
            out[k], out[up] = lora[up], lora[k]
    return out


def _masks_with_one_replaced(c, masks):
    """The first two adapted modules of input width d: the first reads the second's mask, in both layers."""
    a, b = [nm for nm in c.modules if nm != "down_proj"][:2]
    return {k: (masks[k.replace(a, b)] if k.endswith(a) else v) for k, v in masks.items()}


def _down_mask_at_width_d(c, masks):
    """down_proj's mask drawn for [M, d] and repeated along the columns up to ffn (a generator indexed row * d + col % d)."""
    g = torch.Generator().manual_seed(31000 + c.seed)
    out = dict(masks)
    for l in range(c.layers):
        m = (torch.rand(c.B, c.S, c.hidden, generator=g) >= c.p).double() / (1.0 - c.p)
        out[f"layers.{l}.down_proj"] = m.repeat(1, 1, -(-c.ffn // c.hidden))[..., :c.ffn].contiguous()
    return out


def _middle_row_scored(c):
    _, labels = TC.inputs(c)
    labels = labels.clone()
    labels[1, 1:1 + c.S // 3] = torch.randint(3, c.vocab, (c.S // 3,), generator=torch.Generator().manual_seed(c.seed))
    return labels


# defect -> (the cases that carry the feature, what is run wrong: keywords of train_step_cases.ref_step, `masks` among them)
DEFECTS = {
    "biases zeroed": (lambda c: c.bias != "none", lambda c, m: dict(sd=AW.without_biases(TC.weights(c)[0]))),
    "head-norm weights set to 1": (lambda c: c.norms, lambda c, m: dict(sd=QW.with_unit_norms(TC.weights(c)[0]))),
    "head-norm backward skipped": (lambda c: c.norms, lambda c, m: dict(wrong=("norm_bwd_skipped",))),
    "q's and k's norm vectors swapped": (lambda c: c.norms, lambda c, m: dict(sd=QW.with_swapped_norms(TC.weights(c)[0]))),
    "llama3 rule dropped": (lambda c: c.rope == "llama3", lambda c, m: dict(c_run=TC.without(c, rope_scaling=()))),
    "kv head h % Hkv": (lambda c: c.heads // c.kv_heads > 1, lambda c, m: dict(wrong=("kv_head_mod",))),
    "adapter scale halved": (lambda c: True, lambda c, m: dict(scale=0.5 * c.scale)),
    "input gradient of an attention adapter dropped": (lambda c: True, lambda c, m: dict(wrong=("detach:" + _first(c, "q_proj", "k_proj"),))),
    "input gradient of down_proj's adapter dropped": (lambda c: "down_proj" in c.modules, lambda c, m: dict(wrong=("detach:down_proj",))),
    "gate's and up's B exchanged": (lambda c: c.targets == "all", lambda c, m: dict(lora=_swap_gate_up_B(TC.weights(c)[1]))),
    "one module's mask replaced by another's": (lambda c: c.p > 0, lambda c, m: dict(masks=_masks_with_one_replaced(c, m))),
    "down_proj's mask drawn at width d and tiled": (lambda c: c.p > 0 and "down_proj" in c.modules, lambda c, m: dict(masks=_down_mask_at_width_d(c, m))),
    "the unscored row scored": (lambda c: c.rows == "3x40", lambda c, m: dict(labels=_middle_row_scored(c))),
    "loss mean over all rows": (lambda c: True, lambda c, m: dict(wrong=("mean_over_all_rows",))),
}


@pytest.mark.parametrize("what", list(DEFECTS))
def test_a_planted_defect_misses_the_bars(what):
    carries, mutate = DEFECTS[what]
    cases = [c for c in TC.CASES if carries(c)]
    assert cases, what
    seen = {}
    for c in cases:
        masks, want = base(c)
        kw = mutate(c, masks)
        got = TC.ref_step(c, kw.pop("masks", masks), **kw)
        if c.pieces == "nodx":                                   # judged as the GPU test judges the case: without dx_embeds
            got, want = got[:3] + (None,), want[:3] + (None,)
        r = TC.ratios(c, got, want)
        seen[c.id] = TC.worst(r)
        print(f"SENSITIVITY {what}: {c.id}: worst error / bar {seen[c.id]:.1f}  [{TC.show(r)}]")
    # more than 10 x on a case that carries the feature; on EVERY fp32 or bf16 carrier more than 2 x, so the GPU test fails on that very case.
    # The fp8 bars are 3 x bf16's: their carriers are printed above and not asserted
    firm = {k: v for k, v in seen.items() if "-fp8-" not in k}
    assert max(seen.values()) > 10.0, (what, seen)
    assert firm and min(firm.values()) > 2.0, (what, {k: round(v, 2) for k, v in firm.items() if v <= 2.0})
