"""The two models of tests/golden/g13_qwen3_a.npz / g13_qwen3_b.npz, made from a seeded generator instead of being stored:
tools/make_golden_qwen3.py builds transformers' Qwen3ForCausalLM from them, the tests build the engine from them.  Case "a" has the head
geometry of the Qwen3 sizes the engine accepts (d 512 = 4 heads of 128 over 2 kv heads); case "b" is d 896 = 14 heads of 64 over 2 kv heads: a
query group of 7, and 7 K-groups of 128 over the token step's 8 waves, so one wave is idle.  No projection bias, per-head RMSNorm on q and k.
Draws as in tests/attn_bias_weights.py (projection weights N(0, 1/K), layer norm weights 1 + 0.1 N, embeddings N(0, 0.5^2), LoRA A of std 1/r,
B N(0, 0.05^2)); the head norm weights are 1 + 0.3 N and q's and k's differ, so a skipped weight, a swapped vector or a missing norm moves the
logits by tens of percent.  CPU float32, torch's default (Mersenne) generator."""
from types import SimpleNamespace

import torch

RANK, ALPHA, B, S, STEPS = 8, 16.0, 2, 24, 8

# batch_seed: the first seed of `tools/make_golden_qwen3.py --scan` whose eight greedy steps all have a top-2 margin >= 1e-2
CASES = {
    "a": SimpleNamespace(name="a", hidden=512, heads=4, kv_heads=2, ffn=1024, vocab=512, layers=2, eps=1e-6, theta=1e6, seed=1301, batch_seed=2),
    "b": SimpleNamespace(name="b", hidden=896, heads=14, kv_heads=2, ffn=1152, vocab=512, layers=2, eps=1e-6, theta=1e6, seed=1302, batch_seed=0),
}


def golden_name(c):
    return f"g13_qwen3_{c.name}.npz"


def llama_cfg(c, qk_norm=True):
    from avllm.arch import LlamaCfg
    return LlamaCfg(c.hidden, c.heads, c.layers, c.ffn, c.vocab, c.eps, c.theta, c.kv_heads, (), False, False, qk_norm)


def hf_config_dict(c):
    """config.json of case c as transformers' Qwen3Config writes its fields (what a checkpoint directory holds)."""
    return dict(model_type="qwen3", architectures=["Qwen3ForCausalLM"], hidden_size=c.hidden, intermediate_size=c.ffn, num_hidden_layers=c.layers,
                num_attention_heads=c.heads, num_key_value_heads=c.kv_heads, head_dim=c.hidden // c.heads, vocab_size=c.vocab, rms_norm_eps=c.eps,
                max_position_embeddings=4096, rope_theta=c.theta, tie_word_embeddings=False, attention_bias=False, use_sliding_window=False,
                hidden_act="silu")


def weights(c):
    """(HF-named state dict, LoRA state dict `layers.N.<module>.lora_A|B`) of case c."""
    g = torch.Generator().manual_seed(c.seed)
    n = lambda *shape, std=1.0, mean=0.0: torch.randn(*shape, generator=g) * std + mean
    d, f, hd = c.hidden, c.ffn, c.hidden // c.heads
    dkv = c.kv_heads * hd
    sd = {"model.embed_tokens.weight": n(c.vocab, d, std=0.5), "model.norm.weight": n(d, std=0.1, mean=1.0), "lm_head.weight": n(c.vocab, d, std=d ** -0.5)}
    lora = {}
    for i in range(c.layers):
        p = f"model.layers.{i}."
        for nm, rows in (("q_proj", d), ("k_proj", dkv), ("v_proj", dkv), ("o_proj", d)):
            sd[p + f"self_attn.{nm}.weight"] = n(rows, d, std=d ** -0.5)
            lora[f"layers.{i}.{nm}.lora_A"] = n(RANK, d, std=1.0 / RANK)
            lora[f"layers.{i}.{nm}.lora_B"] = n(rows, RANK, std=0.05)
        sd[p + "self_attn.q_norm.weight"], sd[p + "self_attn.k_norm.weight"] = n(hd, std=0.3, mean=1.0), n(hd, std=0.3, mean=1.0)
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = n(f, d, std=d ** -0.5), n(f, d, std=d ** -0.5)
        sd[p + "mlp.down_proj.weight"] = n(d, f, std=f ** -0.5)
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = n(d, std=0.1, mean=1.0), n(d, std=0.1, mean=1.0)
    return sd, lora


def batch(c, seed=None):
    """(inputs_embeds [B, S, d], labels [B, S] with the first 4 positions unscored) of case c."""
    g = torch.Generator().manual_seed(7000 + (c.batch_seed if seed is None else seed) + c.seed)
    x = (torch.randn(B, S, c.hidden, generator=g) * 0.5).bfloat16().float()      # bf16 values: the bf16 engine reads what the reference read
    labels = torch.randint(0, c.vocab, (B, S), generator=g)
    labels[:, :4] = -100
    return x, labels


NORM_KEYS = ("self_attn.q_norm.weight", "self_attn.k_norm.weight")


def with_unit_norms(sd):
    return {k: (torch.ones_like(v) if k.endswith(NORM_KEYS) else v) for k, v in sd.items()}


def with_swapped_norms(sd):
    swap = {"q_norm": "k_norm", "k_norm": "q_norm"}
    return {k: (sd[k.replace(k.split(".")[-2], swap[k.split(".")[-2]])] if k.endswith(NORM_KEYS) else v) for k, v in sd.items()}


def without_norms(sd):
    return {k: v for k, v in sd.items() if not k.endswith(NORM_KEYS)}
