"""Plain float64 restatements of the memory-bound operations (csrc/norm.hip, elementwise.hip, loss_optim.hip, connector_ops.hip).

Every function takes the inputs exactly as the kernel sees them (a bf16 tensor is upcast, never re-drawn) and computes in `dtype`
(float64 by default).  Passing dtype=torch.float32 evaluates the same formula in fp32 on the host: tests/bars.py derives the fp32 bars from the
distance between the two.  tests/test_refs64_cpu.py pins each restatement to torch's own float64 functional op where one exists, so a
mistake here cannot silently become the yardstick of tests/test_bytemovers_gpu.py.  No function here touches the GPU library."""
import math

import torch

F64 = torch.float64


def _c(t, dtype):
    return None if t is None else t.detach().to("cpu").to(dtype)


# ---------------------------------------------------------------- norms
def layernorm(x, w, b, eps, dtype=F64):
    x, w, b = _c(x, dtype), _c(w, dtype), _c(b, dtype)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * w + b


def rmsnorm_fwd(x, w, eps, dtype=F64):
    """-> (y = w * (x * rstd), rstd [rows]) with rstd = rsqrt(mean x^2 + eps)."""
    x, w = _c(x, dtype), _c(w, dtype)
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return w * (x * rstd), rstd.reshape(-1)


def rmsnorm_bwd(dy, x, w, rstd, dres=None, dtype=F64):
    """dx = dres + rstd * (w dy) - x * rstd^3 * mean(w dy x); rstd is the forward's (as the kernel takes it)."""
    dy, x, w, rstd, dres = _c(dy, dtype), _c(x, dtype), _c(w, dtype), _c(rstd, dtype).reshape(-1, 1), _c(dres, dtype)
    g = w * dy
    dx = rstd * g - x * rstd ** 3 * (g * x).mean(-1, keepdim=True)
    return dx if dres is None else dx + dres


def groupnorm_tokens(x, w, b, groups, eps, act=0, dtype=F64):
    """nn.GroupNorm(groups, C) of the [B, C, T] view of token-major x [B, T, C] (+ activation, ids of avllm.lib.ACT_*)."""
    x, w, b = _c(x, dtype), _c(w, dtype), _c(b, dtype)
    B, T, C = x.shape
    xg = x.view(B, T, groups, C // groups)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((xg - mean) * torch.rsqrt(var + eps)).view(B, T, C) * w + b
    return activation(y, act, dtype=dtype)


# ---------------------------------------------------------------- activations
def activation(x, act, r=None, dtype=F64):
    """act ids: 0 none, 1 GELU (erf), 2 quick-GELU x * sigmoid(1.702 x), 3 SiLU; + residual r."""
    x, r = _c(x, dtype), _c(r, dtype)
    if act == 1:
        y = 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))
    elif act == 2:
        y = x * torch.sigmoid(1.702 * x)
    elif act == 3:
        y = x * torch.sigmoid(x)
    else:
        y = x
    return y if r is None else y + r


def swiglu_fwd(gu, dtype=F64):
    gu = _c(gu, dtype)
    F = gu.shape[1] // 2
    g, u = gu[:, :F], gu[:, F:]
    return g * torch.sigmoid(g) * u


def swiglu_bwd(dh, gu, dtype=F64):
    """-> [dg | du]: du = dh * silu(g), dg = dh * u * sig(g) * (1 + g * (1 - sig(g)))."""
    dh, gu = _c(dh, dtype), _c(gu, dtype)
    F = gu.shape[1] // 2
    g, u = gu[:, :F], gu[:, F:]
    sg = torch.sigmoid(g)
    return torch.cat([dh * u * (sg * (1.0 + g * (1.0 - sg))), dh * (g * sg)], 1)


# ---------------------------------------------------------------- RoPE
def rope_inv_freq(hd, theta, scaling=None, dtype=torch.float32):
    """inv_freq [hd/2].  dtype float32 is HF's own (modeling_rope_utils.py: fp32 arange / hd, fp32 pow); float64 is the exact value.
    scaling = (factor, low_freq_factor, high_freq_factor, original_max_position_embeddings): HF's "llama3" rule."""
    inv = 1.0 / (torch.tensor(theta, dtype=dtype) ** (torch.arange(0, hd, 2, dtype=torch.int64).to(dtype) / hd))
    if scaling:
        factor, low, high, octx = scaling
        wavelen = 2 * math.pi / inv
        low_wl, high_wl = octx / low, octx / high
        inv_l = torch.where(wavelen > low_wl, inv / factor, inv)
        smooth = (octx / wavelen - low) / (high - low)
        smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
        medium = ~(wavelen < high_wl) & ~(wavelen > low_wl)
        inv = torch.where(medium, smoothed, inv_l)
    return inv


def rope_angles(positions, hd, theta, scaling=None, hf=True):
    """[T, hd/2] angles.  hf=True: HF's arithmetic (fp32 inv_freq, fp32 product with the position), which is what the model is held to;
    hf=False: the float64 angle."""
    pos = torch.as_tensor(positions, dtype=torch.int64)
    if hf:
        return pos.to(torch.float32)[:, None] * rope_inv_freq(hd, theta, scaling, torch.float32)[None, :]
    return pos.to(F64)[:, None] * rope_inv_freq(hd, theta, scaling, F64)[None, :]


def rope(x, T, heads, hd, positions, theta, scaling=None, inverse=False, hf=True, dtype=F64):
    """Rotate-half RoPE of x [rows = B * T, heads * hd]; row r sits at positions[r % T].  cos / sin of the angle are taken in float64."""
    x = _c(x, dtype)
    rows = x.shape[0]
    ang = rope_angles(positions, hd, theta, scaling, hf).to(F64)
    cos, sin = ang.cos().to(dtype), ang.sin().to(dtype)
    if inverse:
        sin = -sin
    xv = x.reshape(rows // T, T, heads, hd)
    a, b = xv[..., : hd // 2], xv[..., hd // 2:]
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    return torch.cat([a * c - b * s, b * c + a * s], -1).reshape(rows, heads * hd)


# ---------------------------------------------------------------- cross entropy / argmax
def cross_entropy(logits, labels, grad_scale=1.0, dtype=F64):
    """Shifted causal-LM loss (row (b, t) is scored against labels[b, t + 1]; the last row of a sequence and labels outside [0, V) are not
    scored) -> (row_lse [B*T], loss_sum, count, dlogits [B, T, V] = grad_scale / count * (softmax - onehot) on scored rows, 0 elsewhere and
    everywhere when count == 0)."""
    x = _c(logits, dtype)
    B, T, V = x.shape
    lab = labels.detach().cpu()
    tgt = torch.cat([lab[:, 1:], torch.full((B, 1), -100, dtype=lab.dtype)], 1)
    scored = (tgt >= 0) & (tgt < V)
    lse = torch.logsumexp(x, -1)
    picked = x.gather(-1, tgt.clamp(0, V - 1)[..., None])[..., 0]
    loss_sum = ((lse - picked) * scored).sum()
    count = int(scored.sum())
    g = torch.zeros_like(x)
    if count > 0:
        p = torch.exp(x - lse[..., None])
        onehot = torch.zeros_like(x).scatter_(-1, tgt.clamp(0, V - 1)[..., None], 1.0)
        g = (p - onehot) * scored[..., None] * (grad_scale / count)
    return lse.reshape(-1), loss_sum, count, g


def argmax_rows(x):
    """The kernel's documented rule: the lowest index of the maximum with NaN read as -inf.  That is torch.argmax on every row without NaN; a
    row of all -inf (or of -inf and NaN only) gives 0; the result is always in [0, V).  (torch.argmax itself lets the first NaN win; the
    kernel does not pay a second compare per element for that on the token path.)"""
    x = x.detach().cpu().to(F64)
    key = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    mx = key.max(-1, keepdim=True).values
    return (key == mx).to(torch.int8).argmax(-1)


# ---------------------------------------------------------------- optimizer
def clip_coef(sumsq, max_norm, prescale=1.0):
    """clip_grad_norm_'s coefficient on the prescaled gradient, times the prescale: g_used = g * coef."""
    coef = prescale
    if max_norm > 0:
        coef *= min(1.0, max_norm / (math.sqrt(sumsq) * prescale + 1e-6))
    return coef


def adamw_step(p, g, m, v, lr, step, coef=1.0, b1=0.9, b2=0.95, eps=1e-8, wd=0.01, bc1=None, bc2_sqrt=None):
    """torch.optim.AdamW's single-tensor rule in the kernel comment's order: decoupled decay first, then the moments, then
    p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps).  In place on float64 p, m, v."""
    bc1 = 1.0 - b1 ** step if bc1 is None else bc1
    bc2_sqrt = math.sqrt(1.0 - b2 ** step) if bc2_sqrt is None else bc2_sqrt
    gi = g * coef
    p.mul_(1.0 - lr * wd)
    m.mul_(b1).add_(gi * (1.0 - b1))
    v.mul_(b2).add_(gi * gi * (1.0 - b2))
    p.sub_((lr / bc1) * (m / (v.sqrt() / bc2_sqrt + eps)))


def schedule(step, base_lr, total_steps, warmup_steps=0, b1=0.9, b2=0.95, f32=False):
    """(lr, bc1, bc2_sqrt) of optimizer step `step` (1-based): the lr is the schedule's value at step - 1 (avllm/trainer.py lr_at,
    oracle/avsr_oracle.py cosine_lr).  f32=True evaluates the same formula in fp32 (numpy) the way the kernel is written."""
    if f32:
        import numpy as np
        f = np.float32
        t, total = f(step - 1), f(max(total_steps, 1))
        if warmup_steps > 0:
            w = f(warmup_steps)
            if t < w:
                lr = f(base_lr) * t / w
            else:
                lr = f(base_lr) * max(f(0), f(0.5) * (f(1) + np.cos(f(math.pi) * (t - w) / max(f(1), total - w), dtype=f)))
        else:
            lr = f(base_lr) * (f(1) + np.cos(f(math.pi) * t / total, dtype=f)) * f(0.5)
        bc1 = f(1) - np.power(f(b1), f(step), dtype=f)
        bc2s = np.sqrt(f(1) - np.power(f(b2), f(step), dtype=f), dtype=f)
        return float(lr), float(bc1), float(bc2s)
    t = step - 1
    if warmup_steps > 0:
        if t < warmup_steps:
            lr = base_lr * t / max(1, warmup_steps)
        else:
            lr = base_lr * max(0.0, 0.5 * (1.0 + math.cos(math.pi * (t - warmup_steps) / max(1, total_steps - warmup_steps))))
    else:
        lr = base_lr * (1.0 + math.cos(math.pi * t / max(total_steps, 1))) / 2
    return lr, 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)


def dropout_seed(step, skipped, rank=0):
    return ((step + skipped) * 0x9E3779B1 + rank * 0x85EBCA6B + 12345) & 0xFFFFFFFF


# ---------------------------------------------------------------- movers
def im2col_k3(x, stride):
    """nn.Conv1d(kernel_size 3, padding 1, stride) unfolding of token-major x [B, T, C] -> [B * Tout, 3 C], column kw * C + c."""
    x = x.detach().cpu()
    B, T, C = x.shape
    To = (T - 1) // stride + 1
    xp = torch.zeros(B, T + 2, C, dtype=x.dtype)
    xp[:, 1:T + 1] = x
    idx = torch.arange(To) * stride
    return torch.cat([xp[:, idx + kw] for kw in range(3)], -1).reshape(B * To, 3 * C)


def kv_append(kc, vc, k, v, B, T, pos0):
    """cache[b, pos0 + t, :] = k[b * T + t, :]; returns new caches, everything else as it was."""
    kc, vc = kc.detach().cpu().clone(), vc.detach().cpu().clone()
    d = kc.shape[-1]
    kc[:, pos0:pos0 + T] = k.detach().cpu().reshape(B, T, d)
    vc[:, pos0:pos0 + T] = v.detach().cpu().reshape(B, T, d)
    return kc, vc
