"""tests/token_step_cases.py and the extended tests/refs64_kv8.py checked on the CPU before tests/test_token_step_matrix_gpu.py leans on them:

  * coverage: the case list holds every pair of levels of every two factors, the two named deployments, and at most 24 entries;
  * the reference is tied down: with biases, head norms and adapters it reproduces the stored transformers logits of the g12 and g13 fixtures;
  * headroom: for every case the reference with every stored tensor rounded to bf16 stays within HALF of BF16_LOGITS_REL_L2 of the float64
    reference on the same stored prefix, the same cache form and the same step weights -- so a correct bf16 engine has room under the whole bar
    in every crossed form (a case that had not would get another seed, never another bar);
  * sensitivity: the reference with one feature wrong (a defect of the kind the crossings can hide) misses the bars by more than 10 x on a
    case that carries the feature, and by more than 2 x on every case that carries it -- so the GPU test's bars tell such an engine from a
    correct one on each of those cases.

The fp8 cache and the code-form weights are formats, not defects: their distances from the unquantised reference are printed only."""
import copy
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_bias_weights as AW
import qwen3_weights as QW
import refs64_kv8 as R
import token_step_cases as TC
from bars import BF16_LOGITS_REL_L2, F32_LOGITS_ABS, rel_l2

_BASE = {}


def base(c):
    """Per case, computed once and left unchanged: (step weights, adapters, the stored prefix rows as the R rows see them, tokens, the float64
    step logits).  The prefix rows are the reference's own prefill, rounded to bf16 (the engine's q|k|v buffer) and stored in the case's form."""
    if c.name not in _BASE:
        sd, lora = TC.weights(c)
        x, tokens = TC.inputs(c)
        _, past = TC.ref_prefill(c, sd, lora, x)
        store = TC.store_of(c)
        past = TC.rows_of(c, [(store(R.round_bf16(k)), store(R.round_bf16(v))) for k, v in past])
        sds = TC.step_weights(c, sd)
        _BASE[c.name] = (sds, lora, past, tokens, TC.ref_steps(c, sds, lora, list(past), tokens))
    return _BASE[c.name]


# ---------------------------------------------------------------- coverage
def test_the_case_list_covers_every_pair_of_levels():
    assert len(TC.CASES) <= 24 and len({c.name for c in TC.CASES}) == len(TC.CASES)
    for c in TC.CASES:
        assert all(getattr(c, f) in lv for f, lv in TC.FACTORS.items()), c.id
    assert TC.missing_pairs() == []
    q, l = TC.BY_NAME["qwen3-deployment"], TC.BY_NAME["llama32-deployment"]
    assert (q.hidden, q.weights, q.cache, q.norms, q.step, q.split, q.items, q.group) == (512, "fp8", "fp8", 1, "split2", 2, 4, 4)
    assert (l.hidden, l.heads, l.weights, l.cache, l.rope_scaling, l.step, l.split, l.items, l.group) == (896, 14, "bf16", "fp8", (8.0, 1.0, 4.0, 64), "one", -1, 2, 3)
    # the check itself can fail: of an empty list every pair is missing, of the two deployments alone all but their 45 each
    n = [len(lv) for lv in TC.FACTORS.values()]
    total = (sum(n) ** 2 - sum(k * k for k in n)) // 2
    assert len(TC.missing_pairs([])) == total and total - 90 <= len(TC.missing_pairs(TC.CASES[:2])) < total - 45
    for c in TC.CASES:
        assert c.R <= 16 and c.R == c.items * c.group and (c.shared or c.group == 1)
        src = TC.lineage(c)
        assert torch.equal(src[:, -1], torch.arange(c.R)) and bool((src // c.group == torch.arange(c.R)[:, None] // c.group).all())
        if c.shared:
            assert bool((src != torch.arange(c.R)[:, None]).any()), "the reorders move rows"


# ---------------------------------------------------------------- the reference is tied down
@pytest.mark.parametrize("family,name", [("g12", "q"), ("g12", "l"), ("g13", "a"), ("g13", "b")])
def test_reference_reproduces_the_transformers_fixtures(golden_dir, family, name):
    """Biases (g12: q, k, v; and o), head norms (g13), grouped queries of 2 and 7, adapters on: prefill + seven teacher-forced token steps of
    llama_hidden(store=identity) against the logits transformers wrote."""
    mod = AW if family == "g12" else QW
    c = mod.CASES[name]
    z = np.load(os.path.join(golden_dir, mod.golden_name(c)))
    gold = {k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files}
    sd, lora = mod.weights(c)
    lc = SimpleNamespace(scale=mod.ALPHA / mod.RANK)
    x, toks, want = gold["inputs_embeds"], gold["tokens"], gold["step_logits"]
    past, worst = [None] * c.layers, 0.0
    with torch.no_grad():
        for t in range(mod.STEPS):
            xi = x if t == 0 else sd["model.embed_tokens.weight"][toks[:, t - 1]][:, None]
            h = R.llama_hidden(sd, lora, c, lc, xi, past, 0 if t == 0 else mod.S + t - 1, store=R.identity)
            e = float((h[:, -1] @ sd["lm_head.weight"].double().T - want[:, t].double()).abs().max())
            worst = max(worst, e)
    print(f"{family} {name}: worst |reference - transformers| over {mod.STEPS} steps {worst:.2e}")
    assert worst < F32_LOGITS_ABS
    if family == "g12":                                          # and the bias term is what ties it: without it the same run is far away
        h = R.llama_hidden(AW.without_biases(sd), lora, c, lc, x, [None] * c.layers, 0, store=R.identity)
        assert float((h[:, -1] @ sd["lm_head.weight"].double().T - want[:, 0].double()).abs().max()) > 100 * F32_LOGITS_ABS


def test_defaults_leave_the_reference_as_it_was():
    """rnd=identity, wrong=() and a state dict without biases: bit for bit the arithmetic tests/test_kv8_refs_cpu.py pins."""
    c = TC.BY_NAME["c10"]
    sd, lora = TC.weights(c)
    x, _ = TC.inputs(c)
    nob = {k: v for k, v in sd.items() if not k.endswith(".bias")}
    zero = {k: (torch.zeros_like(v) if k.endswith(".bias") else v) for k, v in sd.items()}
    a = R.llama_hidden(nob, lora, c, c.lora_cfg, x, [None] * c.layers, 0)
    b = R.llama_hidden(zero, lora, c, c.lora_cfg, x, [None] * c.layers, 0, R.mx_store, R.identity, ())
    assert torch.equal(a, b)
    y = torch.randn(64, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    assert torch.equal(R.round_bf16(y), y.float().bfloat16().double()) and torch.equal(R.round_bf16(R.round_bf16(y)), R.round_bf16(y))


# ---------------------------------------------------------------- headroom
@pytest.mark.parametrize("c", TC.CASES, ids=lambda c: c.id)
def test_bf16_roundings_leave_half_the_bar(c):
    sds, lora, past, tokens, want = base(c)
    got = TC.ref_steps(c, sds, lora, list(past), tokens, rnd=R.round_bf16)
    per_step = [rel_l2(got[:, t], want[:, t]) for t in range(TC.NEW)]
    print(f"HEADROOM {c.id}: bf16-rounded vs float64 reference, relative L2 per step " + " ".join(f"{e:.2e}" for e in per_step)
          + f"; worst {max(per_step) / BF16_LOGITS_REL_L2:.3f} of the bar")
    assert max(per_step) < 0.5 * BF16_LOGITS_REL_L2
    # the formats themselves, printed only: the case's cache form and step weights against the unquantised reference on the unstored prefix
    if c.cache == "fp8" or c.weights != "bf16":
        sd, _ = TC.weights(c)
        x, _ = TC.inputs(c)
        _, p0 = TC.ref_prefill(c, sd, lora, x)
        plain = TC.ref_steps(c, sd, lora, TC.rows_of(c, p0), tokens, store=R.identity)
        print(f"FORMAT {c.id}: weights {c.weights}, cache {c.cache}: relative L2 from the unquantised reference {rel_l2(want, plain):.3e}")


# ---------------------------------------------------------------- sensitivity
def _without(c, **kw):
    d = copy.copy(c)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _late(past):
    """The cache a writer that is one position late leaves before the first step: the first generated position unwritten (zeros)."""
    return [(torch.cat([k, torch.zeros_like(k[:, :, :1])], 2), torch.cat([v, torch.zeros_like(v[:, :, :1])], 2)) for k, v in past]


# mutation -> (the cases that carry the feature, what is run wrong)
MUTATIONS = {
    "biases zeroed": (lambda c: c.bias != "none", lambda c, sds: dict(sd_steps=AW.without_biases(sds))),
    "norm weights set to 1": (lambda c: c.norms, lambda c, sds: dict(sd_steps=QW.with_unit_norms(sds))),
    "llama3 rule dropped": (lambda c: c.rope == "llama3", lambda c, sds: dict(c_run=_without(c, rope_scaling=()))),
    "kv head h % Hkv": (lambda c: c.heads // c.kv_heads > 1, lambda c, sds: dict(wrong=("kv_head_mod",))),
    "parents not applied": (lambda c: c.shared, lambda c, sds: dict(reorder=False)),
    "row stored one position late": (lambda c: True, lambda c, sds: dict(wrong=("attend_before_append",), late=True)),
    "RoPE at pos instead of S + pos": (lambda c: c.shared, lambda c, sds: dict(rope_base=0)),
    "adapter scale halved": (lambda c: c.lora, lambda c, sds: dict(lc=SimpleNamespace(scale=0.5 * c.lora_cfg.scale))),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_a_wrong_feature_misses_the_bars_tenfold(what):
    carries, mutate = MUTATIONS[what]
    cases = [c for c in TC.CASES if carries(c)]
    assert cases, what
    seen = {}
    for c in cases:
        sds, lora, past, tokens, want = base(c)
        kw = mutate(c, sds)
        start = _late(past) if kw.pop("late", False) else list(past)
        got = TC.ref_steps(c, kw.pop("sd_steps", sds), lora, start, tokens, **kw)
        seen[c.id] = max(max(TC.ratios(got[:, t], want[:, t])) for t in range(TC.NEW))
        print(f"SENSITIVITY {what}: {c.id}: worst error / bar over the steps {seen[c.id]:.1f}")
    # more than 10 x on a case that carries the feature; and on EVERY case that carries it more than 2 x: the half bar that roundings may use
    # (the headroom test) cannot bring such an error back under the bar, so the GPU test fails on that very case
    assert max(seen.values()) > 10.0, (what, seen)
    assert min(seen.values()) > 2.0, (what, {k: round(v, 1) for k, v in seen.items() if v <= 2.0})
