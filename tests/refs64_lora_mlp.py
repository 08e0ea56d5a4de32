"""Float64 torch statement of the Llama decoder with LoRA adapters on any subset of q, k, v, o, gate, up, down (lora_target_modules), with
optional dropout masks, and the inputs the CPU file (tests/test_lora_targets_cpu.py) and the GPU file (tests/test_lora_mlp_gpu.py) share.

Written out here -- RMSNorm, RoPE (rotate-half), causal softmax attention, SwiGLU, the shifted cross entropy -- and tied to the pinned oracle by
the CPU control: with the four default targets it equals oracle.avsr_oracle.llama_hidden / train_step_grads.  Gradients come by autograd,
d loss / d x among them.  Everything is made from seeds on the CPU; nothing here touches the GPU.

tests/train_step_cases.py runs the training-step matrix on the same decoder: projection biases and per-head q/k norms where the state dict
has them, the "llama3" RoPE rule where c.rope_scaling is set, `proj` for the frozen products in another arithmetic (fp8_proj), `rnd` for a model
of the bf16 engine's roundings, `wrong` for planted defects.  With the defaults nothing of this changes a bit of what the functions returned
before (tests/test_train_step_cases_cpu.py keeps a copy of the former decoder and compares).

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


def adapted(x, w, lora, key, scale, masks, bias=None, proj=None, rnd=None, wrong=()):
    """One adapted projection.  bias: the frozen projection's bias (added to the base product, as peft's base_layer does); proj: the frozen
    product in another arithmetic (default x @ w.T), the adapter term stays what it is; rnd: applied to the rank-side product, which the
    engine stores; wrong: "detach:<module>" cuts the adapter branch's input gradient of that module."""
    y = x @ w.T if proj is None else proj(x, w)
    if bias is not None:
        y = y + bias
    if lora is not None and key + ".lora_A" in lora:
        xl = x * masks[key].to(x.dtype).view_as(x) if masks is not None and key in masks else x
        if "detach:" + key.split(".")[-1] in wrong:
            xl = xl.detach()
        t = xl @ lora[key + ".lora_A"].T
        y = y + scale * ((t if rnd is None else rnd(scale * t) / scale) @ lora[key + ".lora_B"].T)
    return y


class _LinearFp8(torch.autograd.Function):
    """oracle.avsr_oracle._LinearFp8 restated for float64 tensors (the oracle's own takes float32 only): forward oracle.mxfp8.linear_fp8 -- both
    operands rounded to bf16 and block-quantised by the MX rule, whose values float32 holds exactly -- with the products summed in float64;
    backward dx = dy W on the unquantised weights, nothing quantised."""

    @staticmethod
    def forward(ctx, x, w):
        from oracle import mxfp8
        ctx.save_for_backward(w)
        fq = lambda t: mxfp8.fake_quant(t.to(torch.bfloat16).float()).to(F64)      # noqa: E731
        return fq(x) @ fq(w).T

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        return dy @ w, None


def fp8_proj(x, w):
    """The frozen product of the fp8 training forward (the `proj` of hidden / step for precision fp8)."""
    return _LinearFp8.apply(x, w)


def head_norm(x, w, eps, straight_through=False):
    """Per-head RMSNorm (Qwen3) over the last axis.  straight_through: the planted defect of a skipped backward (value of the norm, gradient of
    the identity)."""
    y = rms_norm(x, w, eps)
    return x + (y - x).detach() if straight_through else y


def hidden(sd, lora, c, scale, x, masks=None, past=None, pos0=0, proj=None, rnd=None, wrong=()):
    """Final-norm output [B, T, d].  past: optional list of (k, v) per layer, extended in place (a KV cache).
    Projection biases (`<module>.bias`) and per-head q/k norms (`self_attn.q_norm.weight` / `k_norm.weight`, before RoPE) are applied where the
    state dict has them; c.rope_scaling, where set, selects the "llama3" frequency rule (oracle.avsr_oracle.rope_cos_sin, the fp32 table).
    proj: the arithmetic of the frozen products q|k|v, o, gate|up, down (fp8_proj for the fp8 training forward).
    rnd: applied wherever the engine stores a tensor (refs64_kv8.round_bf16: a model of the bf16 engine's roundings; forward only).
    wrong: planted defects for tests/test_train_step_cases_cpu.py -- "kv_head_mod" (query head h reads kv head h % Hkv), "norm_bwd_skipped",
    "detach:<module>" (see adapted).  With the defaults this is the arithmetic it was before any of these existed, bit for bit."""
    B, T, d = x.shape
    H, hd = c.heads, getattr(c, "head_dim", None) or c.hidden // c.heads
    Hkv = getattr(c, "kv_heads", 0) or H
    scaling = tuple(getattr(c, "rope_scaling", ()) or ())
    if scaling:
        from oracle import avsr_oracle as O
        cos, sin = (t.to(F64) for t in O.rope_cos_sin(torch.arange(pos0, pos0 + T), hd, c.theta, scaling))
    else:
        cos, sin = rope_table(pos0, T, hd, c.theta)
    r = (lambda t: t) if rnd is None else rnd
    kw = dict(proj=proj, rnd=rnd, wrong=wrong)
    for i in range(c.layers):
        P, K = f"model.layers.{i}.", f"layers.{i}."
        b = lambda nm: sd.get(P + f"self_attn.{nm}.bias")
        h = r(rms_norm(x, sd[P + "input_layernorm.weight"], c.eps))
        sp = lambda t, n: t.view(B, T, n, hd).transpose(1, 2)
        q = sp(r(adapted(h, sd[P + "self_attn.q_proj.weight"], lora, K + "q_proj", scale, masks, b("q_proj"), **kw)), H)
        k = sp(r(adapted(h, sd[P + "self_attn.k_proj.weight"], lora, K + "k_proj", scale, masks, b("k_proj"), **kw)), Hkv)
        v = sp(r(adapted(h, sd[P + "self_attn.v_proj.weight"], lora, K + "v_proj", scale, masks, b("v_proj"), **kw)), Hkv)
        if P + "self_attn.q_norm.weight" in sd:
            st = "norm_bwd_skipped" in wrong
            q, k = head_norm(q, sd[P + "self_attn.q_norm.weight"], c.eps, st), head_norm(k, sd[P + "self_attn.k_norm.weight"], c.eps, st)
        q, k = r(rope(q, cos, sin)), r(rope(k, cos, sin))
        if past is not None:
            if past[i] is not None:
                k, v = torch.cat([past[i][0], k], dim=2), torch.cat([past[i][1], v], dim=2)
            past[i] = (k, v)
        if Hkv != H and "kv_head_mod" in wrong:
            k, v = k.repeat(1, H // Hkv, 1, 1), v.repeat(1, H // Hkv, 1, 1)
        elif Hkv != H:
            k, v = k.repeat_interleave(H // Hkv, dim=1), v.repeat_interleave(H // Hkv, dim=1)
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        Tk = k.shape[2]
        s = s.masked_fill(~torch.ones(T, Tk, dtype=torch.bool).tril(diagonal=Tk - T), float("-inf"))
        a = r((torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, d))
        x = r(x + adapted(a, sd[P + "self_attn.o_proj.weight"], lora, K + "o_proj", scale, masks, b("o_proj"), **kw))
        h = r(rms_norm(x, sd[P + "post_attention_layernorm.weight"], c.eps))
        g = r(adapted(h, sd[P + "mlp.gate_proj.weight"], lora, K + "gate_proj", scale, masks, **kw))
        u = r(adapted(h, sd[P + "mlp.up_proj.weight"], lora, K + "up_proj", scale, masks, **kw))
        x = r(x + adapted(r(g * torch.sigmoid(g) * u), sd[P + "mlp.down_proj.weight"], lora, K + "down_proj", scale, masks, **kw))
    return r(rms_norm(x, sd["model.norm.weight"], c.eps))


def shifted_ce(logits, labels, wrong=()):
    """HF's causal LM loss: position t predicts label t + 1, -100 ignored, mean over the scored positions.
    wrong: "mean_over_all_rows" divides the scored positions' sum by B * T instead (a planted defect)."""
    B, T, V = logits.shape
    tgt = torch.cat([labels[:, 1:], torch.full((B, 1), -100, dtype=labels.dtype)], dim=1).reshape(-1)
    keep = tgt != -100
    lp = torch.log_softmax(logits.reshape(-1, V)[keep], dim=-1)
    if "mean_over_all_rows" in wrong:
        return -lp.gather(1, tgt[keep][:, None]).sum() / (B * T)
    return -lp.gather(1, tgt[keep][:, None]).mean()


def to64(sd):
    return {k: v.to(F64) for k, v in sd.items()}


def step(sd, lora, c, scale, x, labels, masks=None, proj=None, wrong=()):
    """-> (loss, logits [B, T, V], {adapter tensor: gradient}, d loss / d x), all float64.  proj, wrong: see hidden (proj takes lm_head too)."""
    sd, x = to64(sd), x.to(F64).clone().requires_grad_(True)
    lora = {k: v.to(F64).clone().requires_grad_(True) for k, v in lora.items()}
    xf = hidden(sd, lora, c, scale, x, masks, proj=proj, wrong=wrong)
    logits = xf @ sd["lm_head.weight"].T if proj is None else proj(xf, sd["lm_head.weight"])
    loss = shifted_ce(logits, labels, wrong)
    loss.backward()
    return loss.detach(), logits.detach(), {k: v.grad for k, v in lora.items()}, x.grad


def logits64(sd, lora, c, scale, x, masks=None, proj=None, rnd=None):
    with torch.no_grad():
        sd = to64(sd)
        xf = hidden(sd, None if lora is None else to64(lora), c, scale, x.to(F64), masks, proj=proj, rnd=rnd)
        return xf @ sd["lm_head.weight"].T if proj is None else proj(xf, sd["lm_head.weight"])


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
