"""The two models of tests/golden/g12_attn_bias.npz, made from a seeded generator instead of being stored: tools/make_golden_qwen2.py builds
the transformers models from them, the tests build the engine from them.  Case "q" is a 2-layer Qwen2 with the attention geometry of
Qwen2.5-0.5B (d 896 = 14 heads of 64 over 2 kv heads: a query group of 7, and 7 K-groups of 128 over the token step's 8 waves, so one wave is
idle), biases on q, k, v; case "l" is a Llama saved with attention_bias (d 512 = 4 heads of 128 over 2 kv heads), biases on q, k, v and o.
Draws: projection weights N(0, 1/K), biases N(0, 0.3^2) (Qwen's k biases are large: the term must not be a rounding afterthought), norm
weights 1 + 0.1 N, embeddings N(0, 0.5^2), LoRA A "N(0, 1/r)" in the sense of peft's gaussian init and arch.synth_lora, i.e. std 1/r (with
std r^-0.5 the adapter term is three times the base product, q and k triple, the softmax saturates and transformers' own bf16 run of the
model is 5 % away from its fp32 run: a model no bf16 bar can be stated for), B N(0, 0.05^2): the adapter term is about as large as the base
product, so a misplaced one cannot hide.  CPU float32, torch's default (Mersenne) generator."""
from types import SimpleNamespace

import torch

RANK, ALPHA, B, S, STEPS = 8, 16.0, 2, 24, 8

CASES = {
    "q": SimpleNamespace(name="q", hidden=896, heads=14, kv_heads=2, ffn=1152, vocab=512, layers=2, eps=1e-6, theta=1e6, qkv_bias=True,
                         o_bias=False, seed=1201, batch_seed=0),
    "l": SimpleNamespace(name="l", hidden=512, heads=4, kv_heads=2, ffn=1024, vocab=512, layers=2, eps=1e-5, theta=10000.0, qkv_bias=True,
                         o_bias=True, seed=1202, batch_seed=0),
}


def golden_name(c):
    return "g12_attn_bias.npz" if c.name == "q" else f"g12_attn_bias_{c.name}.npz"


def llama_cfg(c):
    from avllm.arch import LlamaCfg
    return LlamaCfg(c.hidden, c.heads, c.layers, c.ffn, c.vocab, c.eps, c.theta, c.kv_heads, (), c.qkv_bias, c.o_bias)


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
        for nm, rows, has in (("q_proj", d, c.qkv_bias), ("k_proj", dkv, c.qkv_bias), ("v_proj", dkv, c.qkv_bias), ("o_proj", d, c.o_bias)):
            sd[p + f"self_attn.{nm}.weight"] = n(rows, d, std=d ** -0.5)
            if has:
                sd[p + f"self_attn.{nm}.bias"] = n(rows, std=0.3)
            lora[f"layers.{i}.{nm}.lora_A"] = n(RANK, d, std=1.0 / RANK)
            lora[f"layers.{i}.{nm}.lora_B"] = n(rows, RANK, std=0.05)
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


def without_biases(sd):
    return {k: (torch.zeros_like(v) if k.endswith("_proj.bias") else v) for k, v in sd.items()}
