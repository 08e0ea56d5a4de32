"""The token step (csrc/engine.hip llama_decode_layer_fused) across pairings of model forms: the case table, the weights of a case and the
float64 run of a case on tests/refs64_kv8.py.  Pure CPU, everything from seeds: tests/test_token_step_cases_cpu.py checks the table and the
reference on the host, tests/test_token_step_matrix_gpu.py runs every case on the engine.

Ten factors pick the launches of one token step.  CASES is an explicit list that holds every pair of levels of every two factors at least once
(a pairwise covering array: an error that needs two settings to meet -- a bias dropped when the projection goes raw, a suffix row indexed with
the prefix stride, H / Hkv taken from the wrong side under a shared prefix -- is met by some case), and the two deployments the documents name.

A case: a 2-layer model of vocab 512 drawn as tests/qwen3_weights.py and tests/attn_bias_weights.py draw theirs (projections N(0, 1/K), biases
N(0, 0.3^2), head norms 1 + 0.3 N with q's and k's different, layer norms 1 + 0.1 N, embeddings N(0, 0.5^2), LoRA A of std 1/r and B
N(0, 0.05^2) at alpha = 2 r), every tensor rounded to bf16 and held as float32, so the bf16 engine and the float64 reference hold the same
numbers; a prefix of S = 37 positions per item and NEW = 5 teacher-forced tokens per row.  In shared-prefix cases the rows of an item are
reordered between steps (parents()), on the engine's caches and on the reference's `past` alike."""
from types import SimpleNamespace

import torch

import refs64_kv8 as R

S, NEW, LAYERS, VOCAB, EPS = 37, 5, 2, 512, 1e-6
PAD = 2                                                          # cache positions allocated past the last written one: they must keep their fill

GEOMETRY = {"d512": (512, 4, 2, 1024),                           # hidden, heads, kv heads, ffn: 4 x 128 over 2 kv heads, a query group of 2
            "d896": (896, 14, 2, 1152),                          # 14 x 64 over 2 kv heads: a group of 7, 7 K-groups of 128 over the step's 8 waves (one idle)
            "d256": (256, 2, 2, 512)}                            # 2 x 128, kv_heads = heads
ROPE = {"1e4": (1e4, ()), "1e6": (1e6, ()), "llama3": (5e5, (8.0, 1.0, 4.0, 64))}
COPY_ROWS = (1, 3, 16)                                           # rows level 0 / 1 / 2 of a copy-cache case: B
SHARED_ROWS = ((1, 2), (2, 3), (4, 4))                           # ... of a shared-prefix case: (items, rows per item)
SPLIT = {"one": -1, "split2": 2}                                 # knob SHARED_SPLIT of the two shared forms

FACTORS = {"geom": tuple(GEOMETRY), "weights": ("bf16", "fp8", "fp4"), "cache": ("bf16", "fp8"), "norms": (0, 1), "bias": ("none", "qkv", "qkvo"),
           "lora": (0, 8, 16), "rope": tuple(ROPE), "step": ("copy", "one", "split2"), "pos": ("host", "dev"), "rows": (0, 1, 2)}

# name, then the levels in the order of FACTORS, then the seed.  The first two are the deployments: Qwen3 (head norms, fp8 weights, fp8 cache,
# beams on a shared prefix in the sliced form) and Llama-3.2 (heads of 64 in groups of 7, "llama3" frequencies, fp8 cache, one launch).
# Seeds are 4100 + the row number, except where that draw missed the headroom condition of tests/test_token_step_cases_cpu.py (c07, c09, c14:
# an fp8 cache without head norms and few rows; the first seed of 4100 + row + 100 k under 0.45 of the bar was taken)
_TABLE = (
    ("qwen3-deployment", "d512", "fp8", "fp8", 1, "none", 8, "1e6", "split2", "dev", 2, 4100),
    ("llama32-deployment", "d896", "bf16", "fp8", 0, "none", 0, "llama3", "one", "host", 1, 4101),
    ("c02", "d512", "fp4", "bf16", 0, "qkv", 16, "1e4", "copy", "host", 0, 4102),
    ("c03", "d256", "fp8", "bf16", 0, "qkvo", 8, "llama3", "copy", "dev", 1, 4103),
    ("c04", "d896", "bf16", "bf16", 1, "qkvo", 0, "1e4", "split2", "dev", 0, 4104),
    ("c05", "d256", "bf16", "fp8", 1, "qkv", 16, "1e6", "one", "host", 2, 4105),
    ("c06", "d512", "fp4", "fp8", 1, "qkvo", 8, "llama3", "one", "dev", 0, 4106),
    ("c07", "d896", "fp4", "fp8", 0, "qkv", 16, "1e6", "split2", "dev", 1, 4807),
    ("c08", "d896", "fp4", "bf16", 0, "none", 0, "1e6", "copy", "dev", 2, 4108),
    ("c09", "d256", "fp8", "fp8", 0, "none", 16, "1e4", "split2", "host", 0, 4509),
    ("c10", "d512", "bf16", "fp8", 1, "qkv", 8, "1e4", "copy", "host", 1, 4110),
    ("c11", "d896", "fp8", "bf16", 0, "qkvo", 16, "llama3", "one", "host", 2, 4111),
    ("c12", "d512", "fp8", "fp8", 0, "qkv", 0, "llama3", "split2", "dev", 1, 4112),
    ("c13", "d256", "fp4", "bf16", 1, "none", 0, "1e4", "one", "dev", 2, 4113),
    ("c14", "d896", "fp4", "fp8", 0, "qkvo", 8, "1e6", "copy", "host", 0, 5514),
    # beyond the pairs: head norms on an fp8 cache under a shared prefix at the group of 7 (norm in place, append without rotation, shared
    # attention over images with an idle wave), biases and the "llama3" rule on top
    ("c15", "d896", "fp8", "fp8", 1, "qkv", 16, "llama3", "one", "dev", 2, 4115),
)


def _case(name, *levels_seed):
    *levels, seed = levels_seed
    c = SimpleNamespace(name=name, seed=seed, **dict(zip(FACTORS, levels)))
    c.hidden, c.heads, c.kv_heads, c.ffn = GEOMETRY[c.geom]
    c.theta, c.rope_scaling = ROPE[c.rope]
    c.layers, c.vocab, c.eps = LAYERS, VOCAB, EPS
    c.shared = c.step != "copy"
    c.items, c.group = SHARED_ROWS[c.rows] if c.shared else (COPY_ROWS[c.rows], 1)
    c.R = c.items * c.group
    c.split = SPLIT.get(c.step)
    c.lora_cfg = SimpleNamespace(r=c.lora, alpha=2.0 * c.lora, scale=2.0) if c.lora else None
    c.id = "-".join([name] + [str(v) for v in levels])
    return c


CASES = [_case(*row) for row in _TABLE]
BY_NAME = {c.name: c for c in CASES}


def levels(c):
    return {f: getattr(c, f) for f in FACTORS}


def missing_pairs(cases=None):
    """The (factor, level, factor, level) pairs no case of the list holds."""
    import itertools
    want = {(fa, a, fb, b) for fa, fb in itertools.combinations(FACTORS, 2) for a in FACTORS[fa] for b in FACTORS[fb]}
    for c in CASES if cases is None else cases:
        lv = levels(c)
        want -= {(fa, lv[fa], fb, lv[fb]) for fa, fb in itertools.combinations(FACTORS, 2)}
    return sorted(want, key=str)


# ---------------------------------------------------------------- a case's model and inputs
_WEIGHTS = {}


def weights(c):
    """(HF-named state dict, LoRA state dict `layers.N.<module>.lora_A|B` or None) of case c: bf16 values held as float32.  Cached per case."""
    if c.name in _WEIGHTS:
        return _WEIGHTS[c.name]
    g = torch.Generator().manual_seed(c.seed)
    n = lambda *shape, std=1.0, mean=0.0: (torch.randn(*shape, generator=g) * std + mean).bfloat16().float()      # noqa: E731
    d, f, hd = c.hidden, c.ffn, c.hidden // c.heads
    dkv = c.kv_heads * hd
    sd = {"model.embed_tokens.weight": n(c.vocab, d, std=0.5), "model.norm.weight": n(d, std=0.1, mean=1.0), "lm_head.weight": n(c.vocab, d, std=d ** -0.5)}
    lora = {} if c.lora else None
    for i in range(c.layers):
        p = f"model.layers.{i}."
        for nm, rows in (("q_proj", d), ("k_proj", dkv), ("v_proj", dkv), ("o_proj", d)):
            sd[p + f"self_attn.{nm}.weight"] = n(rows, d, std=d ** -0.5)
            if c.bias == "qkvo" or (c.bias == "qkv" and nm != "o_proj"):
                sd[p + f"self_attn.{nm}.bias"] = n(rows, std=0.3)
            if c.lora:
                lora[f"layers.{i}.{nm}.lora_A"] = n(c.lora, d, std=1.0 / c.lora)
                lora[f"layers.{i}.{nm}.lora_B"] = n(rows, c.lora, std=0.05)
        if c.norms:
            sd[p + "self_attn.q_norm.weight"], sd[p + "self_attn.k_norm.weight"] = n(hd, std=0.3, mean=1.0), n(hd, std=0.3, mean=1.0)
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = n(f, d, std=d ** -0.5), n(f, d, std=d ** -0.5)
        sd[p + "mlp.down_proj.weight"] = n(d, f, std=f ** -0.5)
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = n(d, std=0.1, mean=1.0), n(d, std=0.1, mean=1.0)
    _WEIGHTS[c.name] = (sd, lora)
    return sd, lora


def step_weights(c, sd):
    """The state dict the token steps multiply: sd, or its dequantised code form (the prefill always reads sd)."""
    import dequant_weights as DQ
    return {"bf16": lambda s: s, "fp8": DQ.dequantised, "fp4": DQ.dequantised4}[c.weights](sd)


def llama_cfg(c):
    from avllm.arch import LlamaCfg
    return LlamaCfg(c.hidden, c.heads, c.layers, c.ffn, c.vocab, c.eps, c.theta, c.kv_heads, tuple(c.rope_scaling), c.bias != "none", c.bias == "qkvo",
                    bool(c.norms))


def engine_kwargs(c):
    return {"decode_fp8": c.weights == "fp8", "decode_fp4": c.weights == "fp4", "kv_fp8": c.cache == "fp8"}


def inputs(c):
    """(prefix inputs_embeds [items, S, d], bf16 values; tokens int64 [R, NEW]) of case c."""
    g = torch.Generator().manual_seed(9000 + c.seed)
    x = (torch.randn(c.items, S, c.hidden, generator=g) * 0.5).bfloat16().float()
    return x, torch.randint(0, c.vocab, (c.R, NEW), generator=g)


# reorders inside an item, by group size: a cycle, a parent taken twice (group 3: those of
# test_generate_shared_prefix_gpu.py::test_shared_step_against_the_copy_step)
_PERMS = {1: ([0],), 2: ([1, 0], [0, 0], [1, 1]), 3: ([1, 2, 0], [0, 0, 2], [2, 1, 1]), 4: ([1, 2, 3, 0], [0, 0, 2, 3], [3, 1, 1, 2])}


def parents(c, t):
    """The parent row of every row before step t >= 1 of a shared-prefix case, int64 [R]; None where nothing is reordered."""
    if not c.shared or t == 0:
        return None
    perm = torch.tensor(_PERMS[c.group][t % len(_PERMS[c.group])])
    return (torch.arange(c.R) // c.group) * c.group + perm.repeat(c.items)


def lineage(c):
    """src [R, NEW]: after the last step, generated position j of row r holds what row src[r, j] wrote at step j."""
    src = torch.zeros(c.R, NEW, dtype=torch.int64)
    for t in range(NEW):
        p = parents(c, t)
        if p is not None:
            src = src[p]
        src[:, t] = torch.arange(c.R)
    return src


# ---------------------------------------------------------------- the float64 run of a case
def store_of(c):
    return R.mx_store if c.cache == "fp8" else R.identity


def ref_prefill(c, sd, lora, x):
    """The reference's prefill on the original weights, attention over its own rows -> (logits [items, V], past = the unstored k, v per layer)."""
    past = [None] * c.layers
    with torch.no_grad():
        h = R.llama_hidden(sd, lora, c, c.lora_cfg, x, past, 0, store=R.identity)
        return h[:, -1] @ sd["lm_head.weight"].double().T, past


def rows_of(c, past):
    """An items-row `past` as the R rows of the step see it (each item's prefix `group` times), a fresh list."""
    return [(k.repeat_interleave(c.group, 0), v.repeat_interleave(c.group, 0)) for k, v in past]


def ref_steps(c, sd_steps, lora, past, tokens, rnd=R.identity, wrong=(), c_run=None, lc=None, reorder=True, rope_base=S, store=None):
    """The NEW teacher-forced token steps on `past` (R rows, the STORED prefix rows; extended in place) -> logits [R, NEW, V] float64.
    c_run / lc / reorder / rope_base / wrong: what the sensitivity checks vary (the model description the run believes, the adapters' scale,
    whether the parents are applied, the position of the first new token, llama_hidden's own defects).  store: the case's cache form unless given."""
    cr = c if c_run is None else c_run
    lc = c.lora_cfg if lc is None else lc
    store, out = store_of(c) if store is None else store, []
    with torch.no_grad():
        for t in range(NEW):
            p = parents(c, t) if reorder else None
            if p is not None:
                for i in range(c.layers):
                    past[i] = (past[i][0].index_select(0, p), past[i][1].index_select(0, p))
            h = R.llama_hidden(sd_steps, lora, cr, lc, sd_steps["model.embed_tokens.weight"][tokens[:, t]][:, None], past, rope_base + t, store, rnd, wrong)
            out.append(h[:, -1] @ sd_steps["lm_head.weight"].double().T)
    return torch.stack(out, 1)


def ratios(got, want):
    """(relative L2 / BF16_LOGITS_REL_L2, max abs / (BF16_LOGIT_MAX_ABS max(1, max |want|))) of one logits tensor against its reference."""
    from bars import BF16_LOGIT_MAX_ABS, BF16_LOGITS_REL_L2, rel_l2
    got, want = got.double(), want.double()
    return rel_l2(got, want) / BF16_LOGITS_REL_L2, float((got - want).abs().max()) / (BF16_LOGIT_MAX_ABS * max(1.0, float(want.abs().max())))
