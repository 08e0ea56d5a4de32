"""Float64 restatement of the training objective with label smoothing and the z-loss (include/avllm.h, avllm_ce_smooth_fwd), beside
refs64.cross_entropy, and the bars the GPU tests of the kernels hold it to.  tests/test_loss_refs_cpu.py holds the restatement itself to torch
autograd.  No number here comes from a kernel's output."""
import torch

import bars as Bar

F64 = torch.float64
U = Bar.U32


def smooth_cross_entropy(logits, labels, eps, z, grad_scale=1.0, dtype=F64):
    """Row (b, t) is scored against labels[b, t + 1]; the last row of a sequence and labels outside [0, V) are not scored.  Per scored row
        nll = lse - x_y,  u = lse - mean_v x_v,  q = lse^2,  l = (1 - eps) nll + eps u + z q
    -> (row_lse [B*T], loss_sum = sum l, count, terms = [sum nll, sum u, sum q],
        dlogits [B, T, V] = grad_scale / count * ((1 + 2 z lse) softmax - (1 - eps) onehot - eps / V) on scored rows, 0 elsewhere and everywhere
        when count == 0)."""
    x = logits.detach().cpu().to(dtype)
    B, T, V = x.shape
    lab = labels.detach().cpu()
    tgt = torch.cat([lab[:, 1:], torch.full((B, 1), -100, dtype=lab.dtype)], 1)
    scored = (tgt >= 0) & (tgt < V)
    lse = torch.logsumexp(x, -1)
    picked = x.gather(-1, tgt.clamp(0, V - 1)[..., None])[..., 0]
    nll = (lse - picked) * scored
    u = (lse - x.mean(-1)) * scored
    q = lse * lse * scored
    terms = torch.stack([nll.sum(), u.sum(), q.sum()])
    loss_sum = ((1.0 - eps) * nll + eps * u + z * q).sum()
    count = int(scored.sum())
    g = torch.zeros_like(x)
    if count > 0:
        p = torch.exp(x - lse[..., None])
        onehot = torch.zeros_like(x).scatter_(-1, tgt.clamp(0, V - 1)[..., None], 1.0)
        g = ((1.0 + 2.0 * z * lse[..., None]) * p - (1.0 - eps) * onehot - eps / V) * scored[..., None] * (grad_scale / count)
    return lse.reshape(-1), loss_sum, count, terms, g


PATTERNS = ["all", "none", "last_only", "edge_ids", "beyond_vocab"]


def ce_labels(pat, B, T, V, seed=26):
    """The label patterns of tests/test_bytemovers_gpu.py (ce_labels there, same draw), on the host."""
    lab = torch.randint(0, V, (B, T), generator=torch.Generator(device="cpu").manual_seed(seed))
    if pat == "none":
        lab[:] = -100
    elif pat == "last_only":                                     # the shift scores row T-2 against it; position 0's label is never used
        lab[:] = -100
        lab[:, T - 1] = 1 % V
        lab[0, 0] = 0
    elif pat == "edge_ids":
        lab[:, 0::2] = V - 1
        lab[:, 1::2] = 0
    elif pat == "beyond_vocab":
        lab[:, 1::3] = V
        lab[:, 2::3] = V + 12345
    elif pat != "all":
        raise KeyError(pat)
    return lab


def ce_logits(B, T, V, ld, scale, dtype, seed=25):
    """test_cross_entropy's input: randn * scale in a [B, T, ld] buffer with a +80 spike in the last vector of row (1, 5) (B*T >= 80) and the
    padding columns at the sentinel 7.0, rounded to `dtype`, on the host.  -> (buffer, its [:, :, :V] view)."""
    raw = torch.randn(B, T, ld, generator=torch.Generator(device="cpu").manual_seed(seed)) * scale
    if B * T >= 80:
        raw[1, 5, V - 2] += 80.0
    buf = raw.to(dtype)
    buf[:, :, V:] = 7.0
    return buf, buf[:, :, :V]


def scored_rows(labels, V):
    lab = labels.detach().cpu()
    tgt = torch.cat([lab[:, 1:], torch.full((lab.shape[0], 1), -100, dtype=lab.dtype)], 1)
    return (tgt >= 0) & (tgt < V), tgt


def lse_bar(logits, ref_lse):
    """test_cross_entropy's bar of row_lse: the host's fp32 logsumexp from the same inputs + what __expf adds."""
    V = logits.shape[-1]
    return Bar.fp32_bar(ref_lse, torch.logsumexp(logits.float().cpu(), -1).reshape(-1)) + Bar.ce_lse_expf_term(V)


def sum_bars(logits, labels, eps, z):
    """Bars of (terms [3], loss_sum) for ce_smooth_fwd, built as test_cross_entropy builds its loss_sum bar: count x the per-row bar of a term,
    plus the accumulation of count float atomics in arrival order (atomic_sum_term; every term is >= 0, u too: lse >= max >= mean, so the
    running total stays under the sum).  Per-row bars:
        nll = lse - x_y : lse_bar + one rounding at |lse| + |x|                                   (test_cross_entropy's)
        u = lse - s / V : lse_bar + the fp32 mean's bar (fp32_bar against the host's fp32 mean of the same V values; the kernel's sum has
                          chains of <= ceil(V / (256 VN)) + 13 additions, the division rounds once: inside the factor 4) + one rounding
        q = lse^2       : 2 |lse| lse_bar + one rounding
        l               : (1 - eps) bar_nll + eps bar_u + z bar_q + five roundings (1 - eps, three products, two sums: six, one product and
                          sum may contract) at the size of the terms' magnitudes."""
    x64 = logits.double().cpu()
    V = x64.shape[-1]
    ref_lse, ref_sum, cnt, terms, _ = smooth_cross_entropy(logits, labels, eps, z)
    lb = lse_bar(logits, ref_lse)
    lmax, xmax = float(ref_lse.abs().max()), float(x64.abs().max())
    mean64 = x64.mean(-1).reshape(-1)
    mean_bar = Bar.fp32_bar(mean64, logits.float().cpu().mean(-1).reshape(-1))
    row = [lb + U * (lmax + xmax), lb + mean_bar + U * (lmax + float(mean64.abs().max())), 2.0 * lmax * lb + lb * lb + U * lmax * lmax]
    tb = [cnt * r + Bar.atomic_sum_term(cnt, float(t)) for r, t in zip(row, terms)]
    mags = (1.0 - eps) * float(terms[0]) + eps * float(terms[1]) + z * float(terms[2])           # sum of |terms of l|: every one is >= 0
    per_row_mag = (1.0 - eps) * (lmax + xmax) + eps * (lmax + xmax) + z * lmax * lmax
    loss_bar = cnt * ((1.0 - eps) * row[0] + eps * row[1] + z * row[2] + 6.0 * U * per_row_mag) + Bar.atomic_sum_term(cnt, mags)
    return tb, loss_bar


def grad_bar(logits, labels, eps, z, grad_scale, ref_lse, ref_cnt, lb):
    """Elementwise bar of ce_smooth_bwd: test_cross_entropy's derivation with f = 1 + 2 z lse carried through.  The kernel forms
    ((f p - (1 - eps) onehot) - eps / V) g with its own fp32 lse: p = __expf(x - lse) carries the relative error 3 |a| U + 2 U + lse_bar
    (a = x - lse), f carries 2 z lse_bar + two roundings at |f| + 2 z |lse|, the product f p rounds once; the two subtractions round once
    each at the size of their results, 1 - eps and eps / V once each at their own size; g = grad_scale / count and the last product round as
    in test_cross_entropy (grad_scale to fp32, the division, the product: with the subtraction it counted, four)."""
    x64 = logits.double().cpu()
    B, T, V = x64.shape
    scored, tgt = scored_rows(labels, V)
    lse = ref_lse.view(B, T, 1)
    a = x64 - lse
    p = a.exp()
    f = 1.0 + 2.0 * z * lse
    oh = torch.zeros_like(x64).scatter_(-1, tgt.clamp(0, V - 1)[..., None], 1.0) * (1.0 - eps)
    d1 = f * p - oh
    d2 = d1 - eps / V
    e = f.abs() * p * (3 * a.abs() * U + 2 * U + lb) + p * (2.0 * z * lb + 2 * U * (f.abs() + 2.0 * z * lse.abs())) + U * (f * p).abs()
    e = e + 2 * U * oh + U * d1.abs() + 2 * U * eps / V + U * d2.abs() + 4 * U * d2.abs()          # eps and z reach the kernel rounded to fp32: one more each
    return (grad_scale / max(ref_cnt, 1)) * scored[..., None].double() * e + Bar.FP32_DENORM
