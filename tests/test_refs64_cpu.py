"""CPU: the float64 restatements of tests/refs64.py against torch's own float64 functional ops (or autograd, or the optimizer), at float64
rounding level.  They are the yardstick of tests/test_bytemovers_gpu.py, so they are pinned where no GPU is needed."""
import math

import pytest
import torch
import torch.nn.functional as F

import refs64 as R

D = torch.float64
TOL = 1e-12          # float64 rounding (2.2e-16) times the O(1e3) operations of a row, on O(1..1e2) values


def rnd(*shape, seed=0, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=D) * scale + offset


def near(a, b, tol=TOL):
    err = float((a - b).abs().max())
    assert err <= tol * max(1.0, float(b.abs().max())), err


@pytest.mark.parametrize("d,offset", [(8, 0.0), (768, 0.0), (2052, 30.0)])
def test_norms_match_torch(d, offset):
    x, w, b = rnd(5, d, seed=1, offset=offset), rnd(d, seed=2, scale=0.1) + 1, rnd(d, seed=3, scale=0.1)
    near(R.layernorm(x, w, b, 1e-5), F.layer_norm(x, (d,), w, b, 1e-5))
    xa = x.clone().requires_grad_(True)
    ref = w * (xa * torch.rsqrt(xa.pow(2).mean(-1, keepdim=True) + 1e-5))
    y, rstd = R.rmsnorm_fwd(x, w, 1e-5)
    near(y, ref.detach())
    near(rstd, torch.rsqrt(x.pow(2).mean(-1) + 1e-5))
    dy, dres = rnd(5, d, seed=4), rnd(5, d, seed=5)
    ref.backward(dy)
    near(R.rmsnorm_bwd(dy, x, w, rstd), xa.grad)
    near(R.rmsnorm_bwd(dy, x, w, rstd, dres), xa.grad + dres)


@pytest.mark.parametrize("C,G,T", [(64, 8, 1), (64, 8, 7), (1024, 32, 37)])
def test_groupnorm_matches_torch(C, G, T):
    x, w, b = rnd(3, T, C, seed=6, offset=100.0, scale=0.1), rnd(C, seed=7, scale=0.1) + 1, rnd(C, seed=8, scale=0.1)
    ref = F.group_norm(x.transpose(1, 2), G, w, b, 1e-5).transpose(1, 2)
    near(R.groupnorm_tokens(x, w, b, G, 1e-5), ref, 1e-9)       # (x - mean) / sigma at mean / sigma = 1e3 costs three of float64's digits
    near(R.groupnorm_tokens(x, w, b, G, 1e-5, act=1), F.gelu(ref), 1e-9)


def test_activations_match_torch():
    x = torch.cat([torch.linspace(-100, 100, 4001, dtype=D), torch.tensor([0.0, -0.0, -88.0, -104.0, 1e-40, -1e-40], dtype=D)])
    r = rnd(x.numel(), seed=9)
    near(R.activation(x, 1), F.gelu(x))
    near(R.activation(x, 3, r), F.silu(x) + r)
    near(R.activation(x, 2), x * torch.sigmoid(1.702 * x))
    near(R.activation(x, 0, r), x + r)
    gu = rnd(7, 24, seed=10, scale=3.0).requires_grad_(True)
    h = F.silu(gu[:, :12]) * gu[:, 12:]
    near(R.swiglu_fwd(gu), h.detach())
    dh = rnd(7, 12, seed=11)
    h.backward(dh)
    near(R.swiglu_bwd(dh, gu), gu.grad)


def test_rope_matches_transformers_llama3_and_rotate_half():
    from transformers import LlamaConfig
    from transformers.modeling_rope_utils import ROPE_INIT_FUNCTIONS
    rs = {"rope_type": "llama3", "factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192}
    try:
        cfg = LlamaConfig(hidden_size=2048, num_attention_heads=32, num_hidden_layers=1, intermediate_size=64, vocab_size=64, rope_theta=500000.0,
                          rope_scaling=dict(rs), max_position_embeddings=131072)
    except TypeError:
        cfg = LlamaConfig(hidden_size=2048, num_attention_heads=32, num_hidden_layers=1, intermediate_size=64, vocab_size=64,
                          rope_parameters=dict(rs, rope_theta=500000.0), max_position_embeddings=131072)
    inv_hf, att = ROPE_INIT_FUNCTIONS["llama3"](cfg, "cpu")
    assert att == 1.0
    inv = R.rope_inv_freq(64, 500000.0, (32.0, 1.0, 4.0, 8192))
    assert inv.dtype == torch.float32
    assert float(((inv - inv_hf).abs() / inv_hf).max()) <= 2.0 ** -22, "fp32 inv_freq within 2 ulp of transformers'"
    inv64 = R.rope_inv_freq(64, 500000.0, (32.0, 1.0, 4.0, 8192), dtype=D)
    assert float(((inv64 - inv_hf.double()).abs() / inv64).max()) <= 2.0 ** -22
    plain = R.rope_inv_freq(128, 1e4)
    assert torch.equal(plain, 1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.int64).float() / 128)))          # HF's default rule, verbatim
    # the rotation itself: HF's apply_rotary_pos_emb, q * cos + rotate_half(q) * sin, on the same angles
    B, T, H, hd = 2, 19, 3, 64
    x = rnd(B * T, H * hd, seed=12)
    pos = torch.arange(5, 5 + T)
    ang = R.rope_angles(pos, hd, 1e4).double()
    cos, sin = torch.cat([ang, ang], -1).cos()[None, :, None], torch.cat([ang, ang], -1).sin()[None, :, None]
    xv = x.view(B, T, H, hd)
    ref = xv * cos + torch.cat([-xv[..., hd // 2:], xv[..., : hd // 2]], -1) * sin
    out = R.rope(x, T, H, hd, pos, 1e4)
    near(out, ref.reshape(B * T, H * hd))
    near(R.rope(out, T, H, hd, pos, 1e4, inverse=True), x)


@pytest.mark.parametrize("V", [8, 1001])
def test_cross_entropy_matches_torch(V):
    B, T = 3, 11
    x = rnd(B, T, V, seed=13, scale=30.0).requires_grad_(True)
    g = torch.Generator().manual_seed(14)
    labels = torch.randint(0, V, (B, T), generator=g)
    labels[0, 5:] = -100
    labels[1, 3] = V + 7                      # outside the vocabulary: unscored, as the kernel documents
    labels[2, 1], labels[2, 2] = 0, V - 1
    lse, loss_sum, count, grad = R.cross_entropy(x, labels, grad_scale=0.25)
    tgt = torch.cat([labels[:, 1:], torch.full((B, 1), -100)], 1)
    tgt = torch.where(tgt >= V, torch.full_like(tgt, -100), tgt)
    loss = F.cross_entropy(x.view(-1, V), tgt.view(-1), ignore_index=-100, reduction="mean")
    assert count == int((tgt != -100).sum())
    near(loss_sum / count, loss.detach())
    near(lse, torch.logsumexp(x.detach(), -1).reshape(-1))
    (0.25 * loss).backward()
    near(grad, x.grad)
    none = torch.full((B, T), -100)
    none[:, 0] = 3                            # only position 0 labelled: the shift never scores it
    _, ls0, c0, g0 = R.cross_entropy(x, none)
    assert c0 == 0 and float(ls0) == 0.0 and float(g0.abs().max()) == 0.0
    last = torch.full((B, T), -100)
    last[:, T - 1] = 2                        # only the last position labelled: row T - 2 is scored
    assert R.cross_entropy(x, last)[2] == B


def test_argmax_rule_matches_torch():
    ninf, nan = float("-inf"), float("nan")
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0], [ninf, ninf, ninf, ninf], [1.0, nan, 5.0, nan], [float("inf"), 2.0, float("inf"), 0.0],
                      [nan, nan, nan, nan], [-0.0, 0.0, -1.0, 0.0], [ninf, nan, ninf, ninf], [nan, 2.0, 2.0, nan]])
    assert R.argmax_rows(x).tolist() == [1, 0, 2, 0, 0, 0, 0, 1]
    nonan = ~torch.isnan(x).any(-1)
    assert torch.equal(R.argmax_rows(x)[nonan], torch.argmax(x, -1)[nonan])                  # torch's rule wherever no NaN is involved
    assert torch.equal(R.argmax_rows(x), torch.argmax(torch.nan_to_num(x, nan=ninf, posinf=float("inf"), neginf=ninf), -1))      # NaN read as -inf
    assert torch.equal(R.argmax_rows(x.to(torch.bfloat16)), R.argmax_rows(x))


@pytest.mark.parametrize("max_norm,wd", [(0.5, 0.01), (0.0, 0.0), (100.0, 0.01)])
def test_adamw_and_clip_match_torch(max_norm, wd):
    n, steps, lr0 = 257, 12, 3e-3
    p0 = rnd(n, seed=15)
    tp = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([tp], lr=lr0, betas=(0.9, 0.95), eps=1e-8, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    for s in range(1, steps + 1):
        g = rnd(n, seed=100 + s, scale=0.3)
        lr = R.schedule(s, lr0, 40)[0]
        for grp in opt.param_groups:
            grp["lr"] = lr
        tp.grad = g.clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        R.adamw_step(p, g, m, v, lr, s, coef=R.clip_coef(float((g * g).sum()), max_norm), wd=wd)
        near(p, tp.detach(), 1e-11)
    # prescale s: the gradient buffer holds g / s (e.g. a sum over ranks that still has to be averaged); same update
    p2, m2, v2 = p0.clone(), torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    p3, m3, v3 = p0.clone(), torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    g = rnd(n, seed=99)
    R.adamw_step(p2, g, m2, v2, lr0, 1, coef=R.clip_coef(float((g * g).sum()), 0.5), wd=wd)
    g8 = g * 8
    R.adamw_step(p3, g8, m3, v3, lr0, 1, coef=R.clip_coef(float((g8 * g8).sum()), 0.5, prescale=0.125), wd=wd)
    near(p3, p2, 1e-9)                        # (the 1e-6 in clip_grad_norm_'s denominator is not scaled: equal to ~1e-6 * lr)


def test_schedule_matches_trainer_and_oracle():
    from avllm.trainer import ClipWhisperTrainer
    from oracle import avsr_oracle as O
    tr = ClipWhisperTrainer.__new__(ClipWhisperTrainer)
    for warm, total in ((0, 1000), (100, 1000), (0, 7), (5, 5), (50, 20000)):
        tr.learning_rate, tr.warmup_steps, tr.total_steps = 5e-5, warm, total
        for step in (1, 2, 3, warm, warm + 1, warm + 2, total // 2, total, total + 1, 2 * total + 3, 20000):
            if step < 1:
                continue
            lr, bc1, bc2s = R.schedule(step, 5e-5, total, warm)
            assert abs(lr - tr.lr_at(step - 1)) <= 1e-18, (warm, total, step)
            if warm == 0:
                assert abs(lr - O.cosine_lr(5e-5, step - 1, total)) <= 1e-18
            assert bc1 == 1.0 - 0.9 ** step and bc2s == math.sqrt(1.0 - 0.95 ** step)
            lr32 = R.schedule(step, 5e-5, total, warm, f32=True)[0]
            assert abs(lr32 - lr) <= 1e-4 * 5e-5 + 1e-12         # the fp32 form is the same formula (its exact distance is measured in the GPU test)
    assert R.dropout_seed(1, 0) == (0x9E3779B1 + 12345) & 0xFFFFFFFF
    assert R.dropout_seed(3, 2, rank=1) == (5 * 0x9E3779B1 + 0x85EBCA6B + 12345) & 0xFFFFFFFF


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("T", [1, 7, 8])
def test_im2col_k3_is_unfold_order(stride, T):
    B, C = 2, 16
    x = rnd(B, T, C, seed=16)
    To = (T - 1) // stride + 1
    u = F.unfold(x.transpose(1, 2)[:, :, None, :], (1, 3), padding=(0, 1), stride=(1, stride))      # [B, C*3, To], row c*3 + kw
    ref = u.view(B, C, 3, To).permute(0, 3, 2, 1).reshape(B * To, 3 * C)                           # -> column kw*C + c
    assert torch.equal(R.im2col_k3(x, stride), ref)
    w = rnd(5, C, 3, seed=17)
    conv = F.conv1d(x.transpose(1, 2), w, padding=1, stride=stride).transpose(1, 2).reshape(B * To, 5)
    near(R.im2col_k3(x, stride) @ w.permute(0, 2, 1).reshape(5, 3 * C).t(), conv)


def test_kv_append():
    B, T, Tmax, d = 2, 3, 8, 4
    kc, vc = rnd(B, Tmax, d, seed=18), rnd(B, Tmax, d, seed=19)
    k, v = rnd(B * T, d, seed=20), rnd(B * T, d, seed=21)
    k2, v2 = R.kv_append(kc, vc, k, v, B, T, 5)
    assert torch.equal(k2[:, 5:8], k.view(B, T, d)) and torch.equal(v2[:, 5:8], v.view(B, T, d))
    assert torch.equal(k2[:, :5], kc[:, :5]) and torch.equal(v2[:, :5], vc[:, :5])
