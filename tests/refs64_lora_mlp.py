"""Float64 torch statement of the Llama decoder with LoRA adapters on any subset of q, k, v, o, gate, up, down (lora_target_modules), with
optional dropout masks, and the inputs the CPU file (tests/test_lora_targets_cpu.py) and the GPU file (tests/test_lora_mlp_gpu.py) share.

Written out here -- RMSNorm, RoPE (rotate-half), causal softmax attention, SwiGLU, the shifted cross entropy -- and tied to the pinned oracle by
the CPU control: with the four default targets it equals oracle.avsr_oracle.llama_hidden / train_step_grads.  Gradients come by autograd,
d loss / d x among them.  Everything is made from seeds on the CPU; nothing here touches the GPU.

peft lora.Linear on module m: y = x W^T + scale * (dropout_m(x) A^T) B^T, `masks[f"layers.{i}.{m}"]` the module's mask already scaled by
1 / (1 - p), of the shape of the module's INPUT (width d; ffn for down_proj)."""
import math

import torch

from oracle import weights as Wt

F64 = torch.float64
MODULES = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
MLP = MODULES[4:]
# adapters strong enough that a dropped or misplaced term moves the logits by far more than a bf16 bar (the test measures it): a LoRA init
# (A ~ 0.01 / r, B = 0) would pass with the MLP terms missing
A_STD, B_STD = 0.02, 0.3


def shapes(c, r, nm):
    """(A shape, B shape) of module nm: A [r, in], B [out, r]."""
    dkv = (c.kv_heads or c.heads) * c.head_dim
    din = c.ffn if nm == "down_proj" else c.hidden
    dout = {"k_proj": dkv, "v_proj": dkv, "gate_proj": c.ffn, "up_proj": c.ffn}.get(nm, c.hidden)
    return (r, din), (dout, r)


def lora_weights(c, r, targets, seed=0, a_std=A_STD, b_std=B_STD):
    """float32 adapters `layers.{i}.{module}.lora_A|B` for the targets, each tensor from its own seeded stream."""
    sd = {}
    for i in range(c.layers):
        for nm in targets:
            sa, sb = shapes(c, r, nm)
            sd[f"layers.{i}.{nm}.lora_A"] = Wt._randn(f"mlp.lora.{i}.{nm}.A", seed, sa, a_std)
            sd[f"layers.{i}.{nm}.lora_B"] = Wt._randn(f"mlp.lora.{i}.{nm}.B", seed, sb, b_std) if b_std > 0 else torch.zeros(sb)
    return sd


def tiny_llama(ffn=None):
    """Wt.tiny().llama (d 256, ffn 512, 2 layers, V 256), optionally at another ffn, with its weights."""
    c = Wt.tiny().llama
    if ffn is not None:
        c = Wt.LlamaCfg(**{**vars(c), "ffn": ffn})
    return c, Wt.llama_weights(c, seed=5)


def batch(c, B, S, seed=0):
    """(inputs_embeds x [B, S, d] float32, labels [B, S] with a scored span per row)."""
    x = Wt._randn("mlp.x", seed + 97 * B + S, (B, S, c.hidden), 0.5)
    g = torch.Generator().manual_seed(1000 + seed + S)
    labels = torch.full((B, S), -100, dtype=torch.long)
    for b in range(B):
        n = int(torch.randint(S // 4, S // 2, (1,), generator=g))
        labels[b, 1:1 + n] = torch.randint(3, c.vocab, (n,), generator=g)
    return x, labels


# ------------------------------------------------------------------------------------------------ the decoder
def rms_norm(x, w, eps):
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def rope_table(pos0, T, hd, theta):
    """cos, sin [T, hd] as float64 values of the model's fp32 table (HF computes inv_freq and the angles in fp32; so does the oracle)."""
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    fr = torch.arange(pos0, pos0 + T).float()[:, None] * inv[None, :]
    emb = torch.cat([fr, fr], dim=-1)
    return emb.cos().to(F64), emb.sin().to(F64)


def rope(x, cos, sin):
    h = x.shape[-1] // 2
    return x * cos + torch.cat([-x[..., h:], x[..., :h]], dim=-1) * sin


def adapted(x, w, lora, key, scale, masks):
    y = x @ w.T
    if lora is not None and key + ".lora_A" in lora:
        xl = x * masks[key].to(x.dtype).view_as(x) if masks is not None and key in masks else x
        y = y + scale * ((xl @ lora[key + ".lora_A"].T) @ lora[key + ".lora_B"].T)
    return y


def hidden(sd, lora, c, scale, x, masks=None, past=None, pos0=0):
    """Final-norm output [B, T, d].  past: optional list of (k, v) per layer, extended in place (a KV cache)."""
    B, T, d = x.shape
    H, hd = c.heads, c.head_dim
    Hkv = getattr(c, "kv_heads", 0) or H
    cos, sin = rope_table(pos0, T, hd, c.theta)
    for i in range(c.layers):
        P, K = f"model.layers.{i}.", f"layers.{i}."
        h = rms_norm(x, sd[P + "input_layernorm.weight"], c.eps)
        sp = lambda t, n: t.view(B, T, n, hd).transpose(1, 2)
        q = rope(sp(adapted(h, sd[P + "self_attn.q_proj.weight"], lora, K + "q_proj", scale, masks), H), cos, sin)
        k = rope(sp(adapted(h, sd[P + "self_attn.k_proj.weight"], lora, K + "k_proj", scale, masks), Hkv), cos, sin)
        v = sp(adapted(h, sd[P + "self_attn.v_proj.weight"], lora, K + "v_proj", scale, masks), Hkv)
        if past is not None:
            if past[i] is not None:
                k, v = torch.cat([past[i][0], k], dim=2), torch.cat([past[i][1], v], dim=2)
            past[i] = (k, v)
        if Hkv != H:
            k, v = k.repeat_interleave(H // Hkv, dim=1), v.repeat_interleave(H // Hkv, dim=1)
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        Tk = k.shape[2]
        s = s.masked_fill(~torch.ones(T, Tk, dtype=torch.bool).tril(diagonal=Tk - T), float("-inf"))
        a = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, d)
        x = x + adapted(a, sd[P + "self_attn.o_proj.weight"], lora, K + "o_proj", scale, masks)
        h = rms_norm(x, sd[P + "post_attention_layernorm.weight"], c.eps)
        g = adapted(h, sd[P + "mlp.gate_proj.weight"], lora, K + "gate_proj", scale, masks)
        u = adapted(h, sd[P + "mlp.up_proj.weight"], lora, K + "up_proj", scale, masks)
        x = x + adapted(g * torch.sigmoid(g) * u, sd[P + "mlp.down_proj.weight"], lora, K + "down_proj", scale, masks)
    return rms_norm(x, sd["model.norm.weight"], c.eps)


def shifted_ce(logits, labels):
    """HF's causal LM loss: position t predicts label t + 1, -100 ignored, mean over the scored positions."""
    B, T, V = logits.shape
    tgt = torch.cat([labels[:, 1:], torch.full((B, 1), -100, dtype=labels.dtype)], dim=1).reshape(-1)
    keep = tgt != -100
    lp = torch.log_softmax(logits.reshape(-1, V)[keep], dim=-1)
    return -lp.gather(1, tgt[keep][:, None]).mean()


def to64(sd):
    return {k: v.to(F64) for k, v in sd.items()}


def step(sd, lora, c, scale, x, labels, masks=None):
    """-> (loss, logits [B, T, V], {adapter tensor: gradient}, d loss / d x), all float64."""
    sd, x = to64(sd), x.to(F64).clone().requires_grad_(True)
    lora = {k: v.to(F64).clone().requires_grad_(True) for k, v in lora.items()}
    logits = hidden(sd, lora, c, scale, x, masks) @ sd["lm_head.weight"].T
    loss = shifted_ce(logits, labels)
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad for k, v in lora.items()}, x.grad


def logits64(sd, lora, c, scale, x):
    with torch.no_grad():
        sd = to64(sd)
        return hidden(sd, None if lora is None else to64(lora), c, scale, x.to(F64)) @ sd["lm_head.weight"].T


def greedy(sd, lora, c, scale, x, n):
    """n greedy tokens after the prefill of x -> (ids [B, n], top-1 minus top-2 logit of every decision [B, n]), float64, with a KV cache."""
    with torch.no_grad():
        sd, lora = to64(sd), None if lora is None else to64(lora)
        past = [None] * c.layers
        h = hidden(sd, lora, c, scale, x.to(F64), past=past)
        pos, ids, margins = x.shape[1], [], []
        for _ in range(n):
            lg = h[:, -1] @ sd["lm_head.weight"].T
            top = lg.topk(2, dim=-1).values
            ids.append(lg.argmax(-1)); margins.append(top[:, 0] - top[:, 1])
            h = hidden(sd, lora, c, scale, sd["model.embed_tokens.weight"][ids[-1]][:, None], past=past, pos0=pos)
            pos += 1
        return torch.stack(ids, 1), torch.stack(margins, 1)


def merged_sd64(sd, lora, c, scale):
    """The float64 state dict with W + scale * B.A on every adapted module."""
    out = to64(sd)
    for k in lora:
        if k.endswith(".lora_A"):
            _, i, nm, _ = k.split(".")
            key = f"model.layers.{i}.{'mlp' if nm in MLP else 'self_attn'}.{nm}.weight"
            out[key] = out[key] + scale * (lora[k[:-1] + "B"].to(F64) @ lora[k].to(F64))
    return out


def seed_of(base, layers, l, nm):
    """The dropout seed of module nm of layer l (include/avllm.h, avllm_llama.dropout_seed)."""
    j = MODULES.index(nm)
    return (base + 4 * l + j if j < 4 else base + 4 * layers + 3 * l + (j - 4)) & 0xFFFFFFFF
