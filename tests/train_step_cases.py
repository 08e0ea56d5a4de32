"""The training step (csrc/engine.hip avllm_llama_lora_fwd_loss, avllm_llama_lora_bwd_layers_dx) across pairings of model forms: the case table,
the weights and inputs of a case, which launch forms the engine's predicates select for it, and the float64 run of a case on
tests/refs64_lora_mlp.py.  Pure CPU, everything from seeds: tests/test_train_step_cases_cpu.py checks the table and the reference on the host,
tests/test_train_step_matrix_gpu.py runs every case on the engine.

Ten factors pick the launches of one forward + backward.  CASES is an explicit list that holds every pair of levels of every two factors at
least once, except the pairs the engine refuses (IMPOSSIBLE), and starts with the two deployments the documents name.  An error that needs
two settings to meet -- a bias slice offset taken with d where dkv is meant, the head-norm backward reading dqkv after a projection gradient
used it in the unbatched order, down_proj's materialised mask indexed with the wrong width, the second backward piece running the loss
gradient again, an adapter's input gradient lost when only k_proj has one -- is met by some case.  No level of the issue's table is dropped.

A case: a 2-layer model of vocab 512 and eps 1e-6 drawn as tests/token_step_cases.py draws its models (projections N(0, 1/K), biases
N(0, 0.3^2), head norms 1 + 0.3 N with q's and k's different, layer norms 1 + 0.1 N), adapters of the strength of tests/refs64_lora_mlp.py
(A_STD, B_STD, alpha = 2 r, scaled to the width and rank as the comment at A_STD_WIDTH says: a missing adapter term is far outside a bf16
bar), every tensor rounded to the case's engine dtype and held as float32, so the engine and the reference hold the same numbers.

Two things the CPU checks decided in the table: a bf16 case with k_proj as the only attention adapter has rank 16, no head norms, rows 3x40
and geometry g512 (at rank 8 with head norms on 1x333 the planted "input gradient of k_proj's adapter dropped" missed the bars by 1.9 x only,
whatever the seed; the fp32 cases carry the other pairings of k-up-down), and the default deployment runs on rows 3x40 (on 2x256 its
bf16-rounded forward used 0.56 of the logits bar over eight seeds).

What forms() shows cannot vary at these geometries, and why the table is not bent for it:
  * rope_fused (the inverse RoPE inside the attention backward) follows the engine dtype alone: every head dim here is 64 or 128, which is
    also all the head norms accept, so it is true in every bf16 / fp8 case and false in every fp32 one;
  * the at_slice half of the `seg` forms never fails: LlamaEngine always allocates q|k|v's (gate|up's) transposed A images as the slices of one
    matrix, so seg_qkv / seg_gu are "all of the group adapted and no dropout" and a subset goes through lora_dx_dropped with p = 0;
  * mask_fused_f is stated only where it decides something (dropout on and down_proj adapted); it is False elsewhere."""
import copy
import itertools
from types import SimpleNamespace

import torch

import refs64_lora_mlp as R

LAYERS, VOCAB, EPS, P_DROP = 2, 512, 1e-6, 0.25
# Adapter strengths.  refs64_lora_mlp draws A at std A_STD and B at std B_STD for its model of width 256: there the rank-side product x A^T has
# std A_STD * 16 and the term t B^T grows with sqrt(r).  Taken unscaled to these widths and ranks the term grows with sqrt(K r) (1.4 x the base
# product at d 896, rank 16) and the bf16-rounded forward of the CPU headroom check sits at 0.6 .. 1.06 of BF16_LOGITS_REL_L2 whatever the seed
# (six seeds each of three cases): no draw leaves a correct engine half the bar, and at d 896 not even the bar.  So the SIZE of the term is
# held instead: A's std is A_STD * sqrt(192 / K) for an input of width K, B's is B_STD * sqrt(16 / r), alpha = 2 r.  192 and not 256: at 256 the
# rank-32 all-linear case sat at 0.51 .. 0.55 of the bar over five seeds and the default deployment at 0.50; at 192 every case is under 0.46 and
# every planted defect still misses by more than 2.4 x on every fp32 / bf16 carrier (tests/test_train_step_cases_cpu.py prints both).
A_STD_WIDTH, B_STD_RANK = 192, 16

GEOMETRY = {"g512": (512, 4, 2, 1024),                           # hidden, heads, kv heads, ffn: heads of 128 in groups of 2; dkv 256; d, dkv, ffn % 256 == 0
            "g512n": (512, 8, 2, 640),                           # heads of 64 in groups of 4; dkv 128; d % 256 == 0 only: batches the forward, not the backward
            "g896": (896, 14, 2, 1152)}                          # heads of 64 in groups of 7; dkv 128; nothing % 256: batches and fuses nothing
TARGETS = {"attn": R.MODULES[:4], "qv": ("q_proj", "v_proj"), "all": R.MODULES, "k-up-down": ("k_proj", "up_proj", "down_proj")}
ROPE = {"1e4": (1e4, ()), "1e6": (1e6, ()), "llama3": (5e5, (8.0, 1.0, 4.0, 64))}
ROWS = {"2x256": (2, 256), "3x40": (3, 40), "1x333": (1, 333)}

FACTORS = {"geom": tuple(GEOMETRY), "precision": ("fp32", "bf16", "fp8"), "targets": tuple(TARGETS), "rank": (8, 16, 32), "drop": ("off", "host", "dev"),
           "norms": (0, 1), "bias": ("none", "qkv", "qkvo"), "rope": tuple(ROPE), "rows": tuple(ROWS), "pieces": ("whole", "split", "nodx")}

# the pairs LlamaEngine.__init__ / check_llama refuse: the fp8 training forward takes adapters on q, k, v, o only
IMPOSSIBLE = (("precision", "fp8", "targets", "all"), ("precision", "fp8", "targets", "k-up-down"))

# name, then the levels in the order of FACTORS, then the seed (5100 + the row number; no case of this table has needed another draw).  The first two are the
# deployments: the default one (the four attention adapters at rank 16 under dropout from the step-state seed, the backward in two pieces) and
# a Qwen3-style all-linear one (head norms, theta 1e6, all seven modules).  c02 .. c18 complete the pairs (a greedy search, then written out).
_TABLE = (
    ("default-deployment", "g512", "bf16", "attn", 16, "dev", 0, "none", "1e6", "3x40", "split", 5100),
    ("qwen3-all-linear", "g512", "bf16", "all", 8, "host", 1, "none", "1e6", "2x256", "whole", 5101),
    ("c02", "g896", "fp32", "all", 32, "off", 0, "qkv", "1e4", "2x256", "nodx", 5102),
    ("c03", "g512n", "bf16", "all", 16, "dev", 1, "qkvo", "llama3", "3x40", "nodx", 5103),
    ("c04", "g896", "fp32", "k-up-down", 8, "host", 1, "none", "llama3", "1x333", "split", 5104),
    ("c05", "g512n", "fp8", "qv", 32, "dev", 0, "qkv", "1e6", "1x333", "whole", 5105),
    ("c06", "g512", "fp8", "attn", 16, "off", 1, "qkv", "llama3", "1x333", "split", 5106),
    ("c07", "g512", "fp8", "qv", 16, "host", 1, "qkvo", "1e4", "2x256", "nodx", 5107),
    ("c08", "g896", "fp8", "attn", 8, "off", 0, "qkvo", "1e4", "3x40", "whole", 5108),
    ("c09", "g512", "fp32", "k-up-down", 32, "off", 1, "qkvo", "1e6", "3x40", "whole", 5109),
    ("c10", "g512n", "fp32", "attn", 32, "host", 0, "none", "llama3", "2x256", "nodx", 5110),
    ("c11", "g512n", "fp32", "k-up-down", 16, "dev", 1, "none", "1e4", "2x256", "split", 5111),
    ("c12", "g512n", "bf16", "qv", 8, "off", 0, "qkv", "llama3", "3x40", "whole", 5112),
    ("c13", "g512", "bf16", "all", 32, "dev", 0, "qkvo", "1e4", "1x333", "split", 5113),
    ("c14", "g896", "fp32", "k-up-down", 8, "dev", 0, "none", "1e6", "1x333", "nodx", 5114),
    ("c15", "g896", "bf16", "qv", 16, "off", 1, "none", "1e6", "2x256", "split", 5115),
    ("c16", "g512", "bf16", "k-up-down", 16, "host", 0, "qkv", "1e4", "3x40", "whole", 5116),
    ("c17", "g512n", "fp32", "qv", 8, "dev", 1, "qkvo", "1e4", "2x256", "split", 5117),
    ("c18", "g512n", "fp8", "qv", 8, "dev", 0, "none", "1e6", "1x333", "split", 5118),
    # beyond the pairs, the crossings the suite had nowhere: a bias with a q/v subset at the group of 7 in bf16 under materialised dropout, the
    # backward in two pieces; head norms with all seven adapters under materialised dropout where nothing batches or fuses
    ("c19", "g896", "bf16", "qv", 16, "host", 0, "qkv", "1e6", "3x40", "split", 5119),
    ("c20", "g896", "bf16", "all", 16, "host", 1, "qkv", "llama3", "1x333", "whole", 5120),
)


def _case(name, *levels_seed):
    *levels, seed = levels_seed
    c = SimpleNamespace(name=name, seed=seed, **dict(zip(FACTORS, levels)))
    c.hidden, c.heads, c.kv_heads, c.ffn = GEOMETRY[c.geom]
    c.head_dim = c.hidden // c.heads
    c.theta, c.rope_scaling = ROPE[c.rope]
    c.layers, c.vocab, c.eps = LAYERS, VOCAB, EPS
    c.B, c.S = ROWS[c.rows]
    c.modules = TARGETS[c.targets]
    c.r, c.scale = c.rank, 2.0
    c.p = 0.0 if c.drop == "off" else P_DROP
    c.id = "-".join([name] + [str(v) for v in levels])
    return c


CASES = [_case(*row) for row in _TABLE]
BY_NAME = {c.name: c for c in CASES}


def variant(c, **levels):
    """Case c with some levels changed (same name stem and seed): the fp32 neighbour of a bf16 case, a case without its biases."""
    lv = dict(levels_of(c), **levels)
    return _case(c.name + "~" + "-".join(f"{k}={v}" for k, v in levels.items()), *[lv[f] for f in FACTORS], c.seed)


def levels_of(c):
    return {f: getattr(c, f) for f in FACTORS}


def missing_pairs(cases=None):
    """The (factor, level, factor, level) pairs no case of the list holds, the IMPOSSIBLE ones left out."""
    want = {(fa, a, fb, b) for fa, fb in itertools.combinations(FACTORS, 2) for a in FACTORS[fa] for b in FACTORS[fb]} - set(IMPOSSIBLE)
    for c in CASES if cases is None else cases:
        lv = levels_of(c)
        want -= {(fa, lv[fa], fb, lv[fb]) for fa, fb in itertools.combinations(FACTORS, 2)}
    return sorted(want, key=str)


# ---------------------------------------------------------------- the launch forms of a case
def forms(c):
    """Which form each predicate of the training step takes for case c, restated from csrc/engine.hip (line numbers of that file).  The engine
    dtype is bf16 in the bf16 and fp8 cases (m->fp8 only switches the frozen products of the FORWARD), fp32 otherwise."""
    d, f, r = c.hidden, c.ffn, c.rank
    dkv = c.kv_heads * c.head_dim
    bf16 = c.precision != "fp32"
    drop = c.p > 0
    has = lambda *ms: all(m + "_proj" in c.modules for m in ms)      # noqa: E731
    batchable = bf16 and r <= 16                                     # av_lora_batch_supported (csrc/lora_batch.hip:243): bf16, 1 <= R <= 16
    fusable_d = bf16 and d % 256 == 0 and r <= 16                    # lora_mask_fusable(m, d), :191
    fusable_f = bf16 and f % 256 == 0 and r <= 16                    # lora_mask_fusable(m, ffn), :191, asked with K = ffn at :441 and :649
    masks_ok = not drop or fusable_d                                 # (dr.p == 0.f || dr.fused), dr = lora_drop(m) at width d, :318-322
    return {
        # :597-598  !fq && bf16 && q, k, v all && masks_ok && d % 256 == 0 && av_lora_batch_supported(dt, r, 3)
        "fwd_qkv_batch": c.precision == "bf16" and has("q", "k", "v") and masks_ok and d % 256 == 0 and batchable,
        # :736-737  the same without !fq, and dkv % 256 == 0
        "bwd_qkv_batch": has("q", "k", "v") and masks_ok and d % 256 == 0 and dkv % 256 == 0 and batchable,
        # :634-635  bf16 && gate && up && masks_ok && d % 256 == 0 && av_lora_batch_supported(dt, r, 2)
        "fwd_gu_batch": has("gate", "up") and masks_ok and d % 256 == 0 and batchable,
        # :466  the same, and f % 256 == 0
        "bwd_gu_batch": has("gate", "up") and masks_ok and d % 256 == 0 and f % 256 == 0 and batchable,
        # :320  lora_drop: {p, p > 0 && lora_mask_fusable(m, K)}; K = d for every module but down_proj
        "mask_fused_d": drop and fusable_d,
        # :441, :649  K = ffn: down_proj's own condition (and :267, the xdf buffer of the materialised form)
        "mask_fused_f": drop and has("down") and fusable_f,
        # :758  any && !drop && contiguous (all three present; at_slice holds for every engine-made image, :367), behind l > 0 || dx_embeds (:756)
        "seg_qkv": has("q", "k", "v") and not drop,
        # :719  o's adapter present && !drop
        "seg_o": has("o") and not drop,
        # :486  gate && up && !drop && both at_slice (:359; LlamaEngine shares one [d, 128] image exactly when both are adapted)
        "seg_gu": has("gate", "up") and not drop,
        # :452  down && !drop
        "seg_down": has("down") and not drop,
        # :726  av_attention_bwd_fuses_rope(dt, hd, 0) = bf16 && hd in (64, 128) (csrc/attention.hip:450, :518)
        "rope_fused": bf16 and c.head_dim in (64, 128),
    }


# ---------------------------------------------------------------- a case's model and inputs
_WEIGHTS = {}


def engine_dtype(c):
    return torch.float32 if c.precision == "fp32" else torch.bfloat16


def weights(c):
    """(HF-named state dict, LoRA state dict `layers.N.<module>.lora_A|B`) of case c: values of the engine dtype held as float32.  Cached."""
    if c.name in _WEIGHTS:
        return _WEIGHTS[c.name]
    g = torch.Generator().manual_seed(c.seed)
    dt = engine_dtype(c)
    n = lambda *shape, std=1.0, mean=0.0: (torch.randn(*shape, generator=g) * std + mean).to(dt).float()      # noqa: E731
    d, f, hd = c.hidden, c.ffn, c.head_dim
    dkv = c.kv_heads * hd
    sd = {"model.embed_tokens.weight": n(c.vocab, d, std=0.5), "model.norm.weight": n(d, std=0.1, mean=1.0), "lm_head.weight": n(c.vocab, d, std=d ** -0.5)}
    lora = {}
    for i in range(c.layers):
        p = f"model.layers.{i}."
        for nm, rows in (("q_proj", d), ("k_proj", dkv), ("v_proj", dkv), ("o_proj", d)):
            sd[p + f"self_attn.{nm}.weight"] = n(rows, d, std=d ** -0.5)
            if c.bias == "qkvo" or (c.bias == "qkv" and nm != "o_proj"):
                sd[p + f"self_attn.{nm}.bias"] = n(rows, std=0.3)
        if c.norms:
            sd[p + "self_attn.q_norm.weight"], sd[p + "self_attn.k_norm.weight"] = n(hd, std=0.3, mean=1.0), n(hd, std=0.3, mean=1.0)
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = n(f, d, std=d ** -0.5), n(f, d, std=d ** -0.5)
        sd[p + "mlp.down_proj.weight"] = n(d, f, std=f ** -0.5)
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = n(d, std=0.1, mean=1.0), n(d, std=0.1, mean=1.0)
        for nm in c.modules:
            sa, sb = R.shapes(c, c.rank, nm)
            lora[f"layers.{i}.{nm}.lora_A"], lora[f"layers.{i}.{nm}.lora_B"] = n(*sa, std=R.A_STD * (A_STD_WIDTH / sa[1]) ** 0.5), n(*sb, std=R.B_STD * (B_STD_RANK / c.rank) ** 0.5)
    _WEIGHTS[c.name] = (sd, lora)
    return sd, lora


def llama_cfg(c):
    from avllm.arch import LlamaCfg
    return LlamaCfg(c.hidden, c.heads, c.layers, c.ffn, c.vocab, c.eps, c.theta, c.kv_heads, tuple(c.rope_scaling), c.bias != "none", c.bias == "qkvo",
                    bool(c.norms))


def lora_cfg(c):
    from avllm.arch import LoraCfg
    return LoraCfg(c.rank, 2.0 * c.rank, tuple(c.modules))


def inputs(c):
    """(inputs_embeds x [B, S, d] in N(0, 0.5^2), values of the engine dtype; labels [B, S] with a scored span per row, as refs64_lora_mlp.batch
    makes them).  3x40 keeps its middle row entirely unscored."""
    g = torch.Generator().manual_seed(9000 + c.seed)
    x = (torch.randn(c.B, c.S, c.hidden, generator=g) * 0.5).to(engine_dtype(c)).float()
    labels = torch.full((c.B, c.S), -100, dtype=torch.long)
    for b in range(c.B):
        n = int(torch.randint(c.S // 4, c.S // 2, (1,), generator=g))
        labels[b, 1:1 + n] = torch.randint(3, c.vocab, (n,), generator=g)
    if c.rows == "3x40":
        labels[1] = -100
    return x, labels


SEED_SPLIT = 0x9E3779B1                                          # `dev` cases: this part of the base seed lives in device memory, the rest in the descriptor


def seeds(c):
    """(the step's base seed, the part passed as `seed`, the part held in the device word or None).  The engine adds the two modulo 2^32."""
    base = (0xBEEF0000 + 7919 * c.seed) & 0xFFFFFFFF
    if c.drop != "dev":
        return base, base, None
    return base, (base - SEED_SPLIT) & 0xFFFFFFFF, SEED_SPLIT


def host_masks(c, seed=0):
    """Bernoulli(1 - p) / (1 - p) masks of every adapted module at its input width, from a host generator: what the CPU checks feed the reference
    (the GPU test feeds it the kernels' own masks)."""
    if c.p == 0:
        return None
    g = torch.Generator().manual_seed(77000 + c.seed + seed)
    out = {}
    for l in range(c.layers):
        for nm in c.modules:
            K = c.ffn if nm == "down_proj" else c.hidden
            out[f"layers.{l}.{nm}"] = (torch.rand(c.B, c.S, K, generator=g) >= c.p).double() / (1.0 - c.p)
    return out


# ---------------------------------------------------------------- the float64 run of a case
def proj_of(c):
    return R.fp8_proj if c.precision == "fp8" else None


def ref_step(c, masks=None, sd=None, lora=None, labels=None, scale=None, c_run=None, wrong=()):
    """The float64 step of case c -> (loss, logits, {adapter tensor: gradient}, dx_embeds).  sd / lora / labels / scale / c_run / wrong: what the
    sensitivity checks vary (a mutated state dict, adapters, labels, adapter scale, the model description the run believes, planted defects)."""
    sd0, lora0 = weights(c)
    x, lab0 = inputs(c)
    return R.step(sd0 if sd is None else sd, lora0 if lora is None else lora, c if c_run is None else c_run, c.scale if scale is None else scale, x,
                  lab0 if labels is None else labels, masks, proj=proj_of(c), wrong=wrong)


def ratios(c, got, ref):
    """Every checked quantity of a step as error / bar -> {quantity: ratio}, the bars of tests/bars.py for the case's precision, applied as
    tests/test_lora_mlp_gpu.py's _check_f32 / _check_bf16 apply them.  got, ref = (loss, logits, {tensor: gradient}, dx_embeds or None).
      fp32: |loss| / F32_LOSS_ABS, max |logits| / F32_LOGITS_ABS, per tensor and dx_embeds max |err| / max |ref| / F32_GRAD_REL_MAX;
      bf16: |loss| / BF16_LOSS_ABS, logits relative L2 / BF16_LOGITS_REL_L2, the whole gradient / BF16_GRAD_REL_L2, per tensor and dx_embeds
            relative L2 / BF16_GRAD_TENSOR_REL_L2;
      fp8 (against the fake-quantised reference): FP8_LOSS_ABS, FP8_LOGITS_REL_L2, and FP8_GRAD_REL_L2 for the whole gradient and for dx_embeds.
            tests/bars.py has no per-tensor fp8 bar and none is made up here: the worst tensor over FP8_GRAD_REL_L2 is reported under
            "tensor (printed)" and is not part of worst().
    The gradient key sets must be equal (asserted here: a missing tensor is not a ratio)."""
    import bars as Bar
    from bars import rel_l2
    loss, logits, grads, dx = got
    rl, rlogits, rg, rdx = ref
    assert set(grads) == set(rg), sorted(set(grads) ^ set(rg))
    keys = sorted(rg)
    out = {}
    if c.precision == "fp32":
        rel_max = lambda a, b: float((a.double() - b).abs().max()) / float(b.abs().max())      # noqa: E731
        out["loss"] = abs(float(loss) - float(rl)) / Bar.F32_LOSS_ABS
        out["logits"] = float((logits.double() - rlogits).abs().max()) / Bar.F32_LOGITS_ABS
        per = {k: rel_max(grads[k], rg[k]) / Bar.F32_GRAD_REL_MAX for k in keys}
        out["tensor"] = max(per.values())
        if dx is not None:
            out["dx_embeds"] = rel_max(dx, rdx) / Bar.F32_GRAD_REL_MAX
    else:
        bf = c.precision == "bf16"
        allg, allr = torch.cat([grads[k].flatten().double() for k in keys]), torch.cat([rg[k].flatten() for k in keys])
        out["loss"] = abs(float(loss) - float(rl)) / (Bar.BF16_LOSS_ABS if bf else Bar.FP8_LOSS_ABS)
        out["logits"] = rel_l2(logits, rlogits) / (Bar.BF16_LOGITS_REL_L2 if bf else Bar.FP8_LOGITS_REL_L2)
        out["grad"] = rel_l2(allg, allr) / (Bar.BF16_GRAD_REL_L2 if bf else Bar.FP8_GRAD_REL_L2)
        per = {k: rel_l2(grads[k], rg[k]) / (Bar.BF16_GRAD_TENSOR_REL_L2 if bf else Bar.FP8_GRAD_REL_L2) for k in keys}
        out["tensor" if bf else "tensor (printed)"] = max(per.values())
        if dx is not None:
            out["dx_embeds"] = rel_l2(dx, rdx) / (Bar.BF16_GRAD_TENSOR_REL_L2 if bf else Bar.FP8_GRAD_REL_L2)
    out["worst tensor"] = max(per, key=per.get)
    return out


def worst(ratio):
    """The largest asserted ratio of ratios()' result."""
    return max(v for k, v in ratio.items() if k not in ("worst tensor", "tensor (printed)"))


def show(ratio):
    return " ".join(f"{k} {v:.3f}" if not isinstance(v, str) else f"({v})" for k, v in ratio.items())


def without(c, **kw):
    d = copy.copy(c)
    for k, v in kw.items():
        setattr(d, k, v)
    return d
