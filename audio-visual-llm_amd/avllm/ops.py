"""Tensor-level wrappers over the op-level C ABI (include/avllm.h).  Tensors only carry pointers/strides;
all arithmetic happens in libavllm.so on the current torch stream."""
from __future__ import annotations

import collections
import ctypes as C
import math
import numbers

import numpy as np
import torch

from . import lib as L


def _ld(t):
    assert t.stride(-1) == 1, "innermost dimension must be contiguous"
    return t.stride(-2) if t.dim() >= 2 else t.shape[-1]


def gemm(A, B, out=None, bias=None, R=None, A2=None, B2=None, act=L.ACT_NONE, alpha=1.0, out_f32=False,
         r_mod=0, remap=None, M=None, a_drop=None, n_valid=0, drop=None, plan=False):
    """out[M,N] = act(alpha*(A.B^T + A2.B2^T) + bias) + R.  A [M,K] (row stride free), B [N,K].
    a_drop=(seed, p): A is replaced by dropout(A) on the fly (bf16, N == 64 only).
    drop=(seed, p): the product (before +R) is multiplied by the dropout mask keep(seed, m*N+n, p)/(1-p) -- the adapter's
    input-gradient GEMM of the training backward (csrc/engine.hip).
    plan=True: nothing runs; returns the name (L.GEMM_KERNELS) of the kernel this call gets."""
    lib = L.load()
    M = A.shape[0] if M is None else M
    N, K = B.shape[0], B.shape[1]
    dt = L.dt_of(A)
    if out is None:
        rows = M if remap is None else (M // remap[0]) * remap[1]
        out = torch.empty(rows, N, device=A.device, dtype=torch.float32 if (out_f32 or dt == L.F32) else A.dtype)
    d = L.GemmDesc()
    d.A, d.B, d.C = L.ptr(A), L.ptr(B), L.ptr(out)
    d.lda, d.ldb, d.ldc = _ld(A), _ld(B), _ld(out)
    d.M, d.N, d.K = M, N, K
    if A2 is not None:
        d.A2, d.B2, d.lda2, d.ldb2, d.K2 = L.ptr(A2), L.ptr(B2), _ld(A2), _ld(B2), B2.shape[1]
    d.bias = L.ptr(bias)
    if R is not None:
        d.R, d.ldr = L.ptr(R), _ld(R)
    d.dtype, d.out_f32, d.act, d.alpha, d.r_mod = dt, int(out_f32), act, alpha, r_mod
    if remap is not None:
        d.g_in, d.g_out, d.g_off = remap
    if a_drop is not None:
        d.a_drop_seed, d.a_drop_p = a_drop[0] & 0xFFFFFFFF, a_drop[1]
    if drop is not None:
        d.drop_seed, d.drop_p = drop[0] & 0xFFFFFFFF, drop[1]
    d.n_valid = n_valid
    if plan:
        k = L.i32()
        L.check(lib.avllm_gemm_plan(C.byref(d), C.byref(k)))
        return L.GEMM_KERNELS[k.value]
    L.check(lib.avllm_gemm(C.byref(d), L.stream_ptr()))
    return out


def gemm_tn(P, Q, out, I=None, J=None, alpha=1.0, drop=None):
    """out[I,J] += alpha * P[:, :I]^T . Q[:, :J]; drop=(seed, p) applies dropout to the wide operand on the fly."""
    lib = L.load()
    I = P.shape[1] if I is None else I
    J = Q.shape[1] if J is None else J
    if drop is not None:
        L.check(lib.avllm_gemm_tn_drop(L.ptr(P), _ld(P), I, L.ptr(Q), _ld(Q), J, P.shape[0], L.ptr(out), _ld(out), alpha,
                                       drop[0] & 0xFFFFFFFF, drop[1], L.dt_of(P), L.stream_ptr()))
        return out
    L.check(lib.avllm_gemm_tn(L.ptr(P), _ld(P), I, L.ptr(Q), _ld(Q), J, P.shape[0], L.ptr(out), _ld(out), alpha,
                              L.dt_of(P), L.stream_ptr()))
    return out


def layernorm(x, w, b, eps=1e-5):
    y = torch.empty_like(x)
    L.check(L.load().avllm_layernorm(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), x.numel() // x.shape[-1], x.shape[-1], eps,
                                     L.dt_of(x), L.stream_ptr()))
    return y


def rmsnorm_fwd(x, w, eps):
    y = torch.empty_like(x)
    rows = x.numel() // x.shape[-1]
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    L.check(L.load().avllm_rmsnorm_fwd(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(rstd), rows, x.shape[-1], eps, L.dt_of(x), L.stream_ptr()))
    return y, rstd


def rmsnorm_bwd(dy, x, w, rstd, dres=None):
    dx = torch.empty_like(x)
    L.check(L.load().avllm_rmsnorm_bwd(L.ptr(dy), L.ptr(x), L.ptr(w), L.ptr(rstd), L.ptr(dres), L.ptr(dx),
                                       x.numel() // x.shape[-1], x.shape[-1], L.dt_of(x), L.stream_ptr()))
    return dx


def rope_(x2d, T, heads, hd, pos0=0, theta=10000.0, inverse=False):
    """In place on a [rows, heads*hd] view (row stride free)."""
    L.check(L.load().avllm_rope(L.ptr(x2d), _ld(x2d), x2d.shape[0], T, heads, hd, pos0, theta, int(inverse), L.dt_of(x2d), L.stream_ptr()))
    return x2d


def rope_table(T, hd, pos0=0, theta=10000.0, pos_dev=None, scaling=None, device="cuda"):
    """cos/sin table f32 [T, hd/2, 2] of positions pos0 (+ *pos_dev, an int32 device tensor of one element) + t (avllm_rope_table), the form
    the engine runs.  scaling = (factor, low_freq_factor, high_freq_factor, original_max_position_embeddings): HF's "llama3" rule."""
    tab = torch.empty(T, hd // 2, 2, device=device, dtype=torch.float32)
    if pos_dev is not None:
        assert pos_dev.dtype == torch.int32 and pos_dev.numel() == 1 and pos_dev.is_cuda
    f, lo, hi, octx = scaling if scaling else (1.0, 1.0, 4.0, 0)
    L.check(L.load().avllm_rope_table(L.ptr(tab), T, hd, pos0, theta, L.ptr(pos_dev), f, lo, hi, int(octx), L.stream_ptr()))
    return tab


def rope_tab_(x2d, T, heads, hd, tab, inverse=False):
    """In place on a [rows, heads*hd] view (row stride free): row r is rotated by table row r % T (avllm_rope_tab)."""
    assert tab.dtype == torch.float32 and tab.is_contiguous() and tab.numel() == T * hd
    L.check(L.load().avllm_rope_tab(L.ptr(x2d), _ld(x2d), x2d.shape[0], T, heads, hd, L.ptr(tab), int(inverse), L.dt_of(x2d), L.stream_ptr()))
    return x2d


def qk_norm_rope_(x2d, T, heads, kv_heads, hd, q_w, k_w, eps, tab, save=False, kc=None, vc=None, pos=0, pos_dev=None):
    """Per-head RMSNorm of the q and k heads + rotary embedding, in place on the first (heads + kv_heads) * hd columns of the [rows, ld] q|k|v
    view x2d (avllm_qk_norm_rope); row r reads table row r % T.  save: -> (pre-norm q|k [rows, (heads + kv_heads) hd], rstd [rows, heads +
    kv_heads] f32).  kc, vc [rows, Tmax, kv_heads hd]: the cache form (T == 1): rotated k and untouched v go to cache row pos (+ *pos_dev)."""
    rows, nqk = x2d.shape[0], heads + kv_heads
    assert tab.dtype == torch.float32 and tab.is_contiguous() and tab.numel() == T * hd and q_w.dtype == x2d.dtype and k_w.dtype == x2d.dtype
    pre = torch.empty(rows, nqk * hd, device=x2d.device, dtype=x2d.dtype) if save else None
    rstd = torch.empty(rows, nqk, device=x2d.device, dtype=torch.float32) if save else None
    if kc is not None:
        assert kc.shape == vc.shape == (rows, kc.shape[1], kv_heads * hd) and kc.is_contiguous() and vc.is_contiguous() and kc.dtype == x2d.dtype
    L.check(L.load().avllm_qk_norm_rope(L.ptr(x2d), _ld(x2d), rows, T, heads, kv_heads, hd, L.ptr(q_w), L.ptr(k_w), eps, L.ptr(tab), L.ptr(pre),
                                        L.ptr(rstd), L.ptr(kc), L.ptr(vc), kc.shape[1] if kc is not None else 0, pos, L.ptr(pos_dev), L.dt_of(x2d),
                                        L.stream_ptr()))
    return pre, rstd


def qk_norm_bwd_(dy2d, heads, kv_heads, hd, q_w, k_w, pre, rstd):
    """In place on the q and k slices of dy2d [rows, ld]: the gradient of the normed pre-RoPE heads -> the gradient of the projections'
    outputs, from qk_norm_rope_'s saves (avllm_qk_norm_bwd)."""
    assert pre.is_contiguous() and rstd.is_contiguous() and rstd.dtype == torch.float32 and pre.dtype == dy2d.dtype
    L.check(L.load().avllm_qk_norm_bwd(L.ptr(dy2d), _ld(dy2d), dy2d.shape[0], heads, kv_heads, hd, L.ptr(q_w), L.ptr(k_w), L.ptr(pre), L.ptr(rstd),
                                       L.dt_of(dy2d), L.stream_ptr()))
    return dy2d


def kv_append(k, v, kc, vc, T, pos0):
    """kc[b, pos0 + t, :] = k[b*T + t, :] and the same for v (avllm_kv_append): k, v [B*T, d] views with one row stride, caches [B, Tmax, d] contiguous."""
    B, Tmax, d = kc.shape
    assert k.shape == (B * T, d) and v.shape == k.shape and _ld(k) == _ld(v) and kc.is_contiguous() and vc.is_contiguous() and vc.shape == kc.shape
    L.check(L.load().avllm_kv_append(L.ptr(k), L.ptr(v), _ld(k), L.ptr(kc), L.ptr(vc), B, T, pos0, Tmax, d, L.dt_of(kc), L.stream_ptr()))


def swiglu_fwd(gu):
    M, F2 = gu.shape
    h = torch.empty(M, F2 // 2, device=gu.device, dtype=gu.dtype)
    L.check(L.load().avllm_swiglu_fwd(L.ptr(gu), L.ptr(h), M, F2 // 2, L.dt_of(gu), L.stream_ptr()))
    return h


def swiglu_bwd(dh, gu):
    dgu = torch.empty_like(gu)
    L.check(L.load().avllm_swiglu_bwd(L.ptr(dh), L.ptr(gu), L.ptr(dgu), gu.shape[0], gu.shape[1] // 2, L.dt_of(gu), L.stream_ptr()))
    return dgu


def swiglu_bwd_h(dh, gu):
    """-> (dgu, h): swiglu_bwd(dh, gu) and, from the same pass over gu, h = silu(g) * u as swiglu_fwd(gu) writes it (avllm_swiglu_bwd_h)."""
    if gu.dim() != 2 or gu.shape[1] % 8 or dh.shape != (gu.shape[0], gu.shape[1] // 2) or dh.dtype != gu.dtype:
        raise ValueError(f"swiglu_bwd_h: gu [M, 2F] with F % 4 == 0 and dh [M, F] of one dtype, got {tuple(gu.shape)} and {tuple(dh.shape)}")
    if not (gu.is_contiguous() and dh.is_contiguous()):
        raise ValueError("swiglu_bwd_h: contiguous tensors")
    dgu = torch.empty_like(gu)
    h = torch.empty_like(dh)
    L.check(L.load().avllm_swiglu_bwd_h(L.ptr(dh), L.ptr(gu), L.ptr(dgu), L.ptr(h), gu.shape[0], gu.shape[1] // 2, L.dt_of(gu), L.stream_ptr()))
    return dgu, h


def attention_plan(B, Tq, Tk, H, hd, causal, dtype, impl=0, kv_heads=None):
    """-> (forward, backward) names (L.ATTN_FORMS) of the kernels avllm_attention_fwd / _bwd give the call; backward None where Tq != Tk."""
    f, b = L.i32(-1), L.i32(-1)
    L.check(L.load().avllm_attention_plan(B, Tq, Tk, H, hd, int(causal), dtype, impl, kv_heads or 0, C.byref(f), C.byref(b)))
    return L.ATTN_FORMS[f.value], (L.ATTN_FORMS[b.value] if b.value >= 0 else None)


def attention_fwd(qkv, B, T, H, hd, causal, scale=None, impl=0, want_lse=True, kv_heads=None, Tk=None, k=None, v=None, out=None, plan=False):
    """qkv [B*T, (H + 2*kv_heads)*hd] fused rows [q | k | v] -> (o [B*T, H*hd], lse [B,H,T]).
    k=, v= (both or neither): separate operands, each a [rows, heads*hd] view with its own row stride; qkv is then q alone [B*T, H*hd] and k, v
    hold B*Tk rows (Tk defaults to T; causal query t sees keys <= t + Tk - T).  out=: a [B*T, H*hd] view to write o into (row stride free).
    plan=True: nothing runs; returns the name (L.ATTN_FORMS) of the kernel this call gets."""
    d = H * hd
    dkv = (kv_heads or H) * hd
    Tk = T if Tk is None else Tk
    assert (k is None) == (v is None) and (k is not None or Tk == T)
    if plan:
        return attention_plan(B, T, Tk, H, hd, causal, L.dt_of(qkv), impl, kv_heads)[0]
    o = torch.empty(B * T, d, device=qkv.device, dtype=qkv.dtype) if out is None else out
    assert o.shape == (B * T, d) and o.dtype == qkv.dtype
    lse = torch.empty(B, H, T, device=qkv.device, dtype=torch.float32) if want_lse else None
    es = qkv.element_size()
    scale = hd ** -0.5 if scale is None else scale
    p = L.ptr(qkv)
    if k is None:
        pk, pv, ldk, ldv = p + d * es, p + (d + dkv) * es, _ld(qkv), _ld(qkv)
    else:
        assert qkv.shape == (B * T, d) and k.shape == (B * Tk, dkv) and v.shape == k.shape and k.dtype == qkv.dtype and v.dtype == qkv.dtype
        pk, pv, ldk, ldv = L.ptr(k), L.ptr(v), _ld(k), _ld(v)
    L.check(L.load().avllm_attention_fwd(p, pk, pv, L.ptr(o), L.ptr(lse), B, T, Tk, H, hd, _ld(qkv), ldk, ldv, _ld(o), scale, int(causal),
                                         L.dt_of(qkv), impl, kv_heads or 0, L.stream_ptr()))
    return o, lse


def attention_fwd_mxq(qkv, B, T, H, hd, scale=None):
    """Short non-causal self-attention (T <= 272, hd 64, bf16) with the output block-scaled to e4m3 in the kernel's epilogue:
    qkv [B*T, 3*H*hd] -> (codes uint8 [B*T, H*hd], layout-0 scale image) == mx_quantize(attention_fwd(...)[0], 0) bit for bit."""
    lib = L.load()
    d = H * hd
    q = torch.empty(B * T, d, device=qkv.device, dtype=torch.uint8)
    s = torch.zeros(lib.avllm_mx_scale_bytes(B * T, d), device=qkv.device, dtype=torch.uint8)
    es = qkv.element_size()
    p = L.ptr(qkv)
    L.check(lib.avllm_attention_fwd_mxq(p, p + d * es, p + 2 * d * es, L.ptr(q), d, L.ptr(s), B, T, H, hd, _ld(qkv), _ld(qkv), _ld(qkv),
                                        float(hd ** -0.5 if scale is None else scale), L.stream_ptr()))
    return q, s


def attention_bwd(qkv, o, dout, lse, B, T, H, hd, causal, scale=None, impl=0, kv_heads=None, rope_tab=None, out=None, plan=False):
    """-> dqkv [dq | dk | dv] in qkv's layout (out=: a view of qkv's shape to write into, row stride free).  rope_tab (ops.rope_table's f32
    [T, hd/2, 2]): the inverse rotary is fused into dq | dk (avllm_attention_bwd_rope: bf16, impl 0, head_dim 64 / 128 only).
    plan=True: nothing runs; returns the name (L.ATTN_FORMS) of the kernels this call gets."""
    if plan:
        return attention_plan(B, T, T, H, hd, causal, L.dt_of(qkv), impl, kv_heads)[1]
    d = H * hd
    dkv = (kv_heads or H) * hd
    dqkv = torch.empty_like(qkv) if out is None else out
    assert dqkv.shape == qkv.shape and dqkv.dtype == qkv.dtype
    delta = torch.empty(B, H, T, device=qkv.device, dtype=torch.float32)
    es = qkv.element_size()
    scale = hd ** -0.5 if scale is None else scale
    p, g = L.ptr(qkv), L.ptr(dqkv)
    args = (p, p + d * es, p + (d + dkv) * es, L.ptr(o), L.ptr(dout), L.ptr(lse), g, g + d * es, g + (d + dkv) * es,
            L.ptr(delta), B, T, H, hd, _ld(qkv), _ld(qkv), _ld(qkv), d, _ld(dqkv), _ld(dqkv), _ld(dqkv),
            scale, int(causal), L.dt_of(qkv), impl, kv_heads or 0)
    if rope_tab is None:
        L.check(L.load().avllm_attention_bwd(*args, L.stream_ptr()))
    else:
        assert rope_tab.dtype == torch.float32 and rope_tab.is_contiguous() and rope_tab.numel() == T * hd
        L.check(L.load().avllm_attention_bwd_rope(*args, L.ptr(rope_tab), L.stream_ptr()))
    return dqkv


def _ce_ld(logits):
    """The one row stride the CE kernels take: logits [B,T,V] must be rows of stride ld >= V, ld % 8 == 0, laid out as a [B*T, ld] matrix."""
    B, T, V = logits.shape
    ld = logits.stride(1) if T > 1 else (logits.stride(0) if B > 1 else (V + 7) // 8 * 8)
    if logits.stride(2) != 1 or (B > 1 and logits.stride(0) != T * ld) or ld < V or ld % 8:
        raise ValueError(f"cross entropy: logits {tuple(logits.shape)} with strides {tuple(logits.stride())} are not [B*T] rows of one stride "
                         "(a multiple of 8, >= V)")
    return ld


def ce_fwd(logits, labels):
    """logits [B,T,V] (row stride free: a [:, :, :V] view of a padded buffer is fine), labels int64 [B,T] (-100 = ignore)
    -> (row_lse [B*T], acc = [loss_sum, count])."""
    B, T, V = logits.shape
    row_lse = torch.empty(B * T, device=logits.device, dtype=torch.float32)
    acc = torch.zeros(2, device=logits.device, dtype=torch.float32)
    L.check(L.load().avllm_ce_fwd(L.ptr(logits), _ce_ld(logits), L.ptr(labels), B, T, V, L.ptr(row_lse), L.ptr(acc), L.ptr(acc) + 4,
                                  L.dt_of(logits), L.stream_ptr()))
    return row_lse, acc


def ce_bwd(logits, labels, row_lse, acc, grad_scale=1.0, out=None):
    """dlogits = grad_scale / count * (softmax - onehot) on scored rows.  The kernel takes ONE row stride for logits and dlogits, so the
    gradient is allocated with the strides of `logits` (torch.empty_like would make a padded view dense); out: a tensor of the same shape,
    dtype and strides to write into; out = logits is the in-place form the engine uses."""
    B, T, V = logits.shape
    ld = _ce_ld(logits)
    if out is None:
        out = torch.empty_strided(logits.shape, logits.stride(), device=logits.device, dtype=logits.dtype)
    elif out.shape != logits.shape or out.stride() != logits.stride() or out.dtype != logits.dtype or out.device != logits.device:
        raise ValueError("ce_bwd: out must have the shape, strides, dtype and device of logits")
    L.check(L.load().avllm_ce_bwd(L.ptr(logits), ld, L.ptr(labels), L.ptr(row_lse), L.ptr(acc) + 4, grad_scale, L.ptr(out),
                                  B, T, V, L.dt_of(logits), L.stream_ptr()))
    return out


def check_loss_options(label_smoothing, z_loss):
    """The ranges of the training objective's two options (include/avllm.h, avllm_ce_smooth_fwd): 0 <= label_smoothing < 1, z_loss >= 0, both
    finite.  Returns them as floats."""
    eps, zeta = float(label_smoothing), float(z_loss)
    if not (0.0 <= eps < 1.0):                                   # a NaN fails both comparisons
        raise ValueError(f"label_smoothing={label_smoothing} must be in [0, 1)")
    if not (0.0 <= zeta < math.inf):
        raise ValueError(f"z_loss={z_loss} must be finite and >= 0")
    return eps, zeta


def ce_smooth_fwd(logits, labels, label_smoothing, z_loss):
    """ce_fwd with label smoothing and the z-loss (avllm_ce_smooth_fwd's rule) -> (row_lse [B*T], acc = [sum of the rows' objective, count],
    terms = the raw sums [nll, lse - mean logit, lse^2] over the scored rows)."""
    eps, zeta = check_loss_options(label_smoothing, z_loss)
    B, T, V = logits.shape
    row_lse = torch.empty(B * T, device=logits.device, dtype=torch.float32)
    acc = torch.zeros(2, device=logits.device, dtype=torch.float32)
    terms = torch.zeros(3, device=logits.device, dtype=torch.float32)
    L.check(L.load().avllm_ce_smooth_fwd(L.ptr(logits), _ce_ld(logits), L.ptr(labels), B, T, V, eps, zeta, L.ptr(row_lse), L.ptr(acc),
                                         L.ptr(acc) + 4, L.ptr(terms), L.dt_of(logits), L.stream_ptr()))
    return row_lse, acc, terms


def ce_smooth_bwd(logits, labels, row_lse, acc, label_smoothing, z_loss, grad_scale=1.0, out=None):
    """dlogits of ce_smooth_fwd's objective, grad_scale / count * ((1 + 2 z_loss lse) softmax - (1 - label_smoothing) onehot - label_smoothing / V)
    on scored rows; strides and `out` as ce_bwd."""
    eps, zeta = check_loss_options(label_smoothing, z_loss)
    B, T, V = logits.shape
    ld = _ce_ld(logits)
    if out is None:
        out = torch.empty_strided(logits.shape, logits.stride(), device=logits.device, dtype=logits.dtype)
    elif out.shape != logits.shape or out.stride() != logits.stride() or out.dtype != logits.dtype or out.device != logits.device:
        raise ValueError("ce_smooth_bwd: out must have the shape, strides, dtype and device of logits")
    L.check(L.load().avllm_ce_smooth_bwd(L.ptr(logits), ld, L.ptr(labels), L.ptr(row_lse), L.ptr(acc) + 4, grad_scale, eps, zeta, L.ptr(out),
                                         B, T, V, L.dt_of(logits), L.stream_ptr()))
    return out


def argmax_rows(logits2d):
    out = torch.empty(logits2d.shape[0], device=logits2d.device, dtype=torch.int64)
    L.check(L.load().avllm_argmax_rows(L.ptr(logits2d), _ld(logits2d), logits2d.shape[0], logits2d.shape[1], L.ptr(out),
                                       L.dt_of(logits2d), L.stream_ptr()))
    return out


def check_sampling(temperature, top_k, top_p):
    """The argument rules of HF's TemperatureLogitsWarper / TopKLogitsWarper / TopPLogitsWarper."""
    if not (float(temperature) > 0.0 and float(temperature) < float("inf")):
        raise ValueError(f"temperature must be a strictly positive float, got {temperature}")
    if not (0.0 < float(top_p) <= 1.0):
        raise ValueError(f"top_p must be a float in (0, 1], got {top_p}")
    if int(top_k) != top_k or int(top_k) < 0:
        raise ValueError(f"top_k must be a non-negative integer, got {top_k}")


def row_scores(logits, tokens, temperature=1.0, entropy=False, logprobs=False):
    """Token scores of float32 logits [rows, V] (row stride free, unit column stride) in one pass (csrc/token_score.hip): the
    log-probability log_softmax(logits / temperature)[r, tokens[r]] of one token per row, float32 [rows], and with entropy=True also the
    entropy of softmax(logits / temperature) per row in nats: returns logprob, or (logprob, entropy).  tokens: int64 [rows] on the
    device; the host cannot check their range without a sync, so the kernel clamps them to [0, V).  tokens=None returns -logsumexp per
    row instead, so that logits[r, v] / temperature + result[r] is the log-probability of any v.  Entries of -inf (banned tokens) carry
    probability 0; a chosen token that is -inf scores -inf; a row of nothing but -inf gives NaN.
    logprobs=True: the rows are log-probabilities already (logits_process(log_softmax=True)): nothing is normalised, temperature is not
    applied, logprob is logits[r, tokens[r]] bit for bit and the entropy is -sum exp(x) * x."""
    if not (torch.is_tensor(logits) and logits.dim() == 2 and logits.is_cuda and logits.stride(1) == 1
            and logits.dtype in (torch.float32, torch.bfloat16)):      # bf16 is refused by the library itself (AV_ERR_UNSUPPORTED)
        raise ValueError("row_scores: logits must be a 2-d float32 device tensor with unit column stride")
    rows, V = logits.shape
    if tokens is not None and not (torch.is_tensor(tokens) and tokens.dtype == torch.int64 and tokens.shape == (rows,) and tokens.is_cuda
                                   and tokens.is_contiguous()):
        raise ValueError(f"row_scores: tokens must be int64 [{rows}] on the device")
    if not logprobs and not (float(temperature) > 0.0 and float(temperature) < float("inf")):
        raise ValueError(f"temperature must be a strictly positive float, got {temperature}")
    lp = torch.empty(rows, device=logits.device, dtype=torch.float32)
    ent = torch.empty(rows, device=logits.device, dtype=torch.float32) if entropy else None
    lib = L.load()
    if logprobs:
        L.check(lib.avllm_row_scores_logprobs(L.ptr(logits), _ld(logits), rows, V, L.ptr(tokens), L.ptr(lp), L.ptr(ent), L.dt_of(logits),
                                              L.stream_ptr()))
    else:
        L.check(lib.avllm_row_scores(L.ptr(logits), _ld(logits), rows, V, L.ptr(tokens), float(temperature), L.ptr(lp), L.ptr(ent),
                                     L.dt_of(logits), L.stream_ptr()))
    return (lp, ent) if entropy else lp


def sample_rows(logits, temperature, top_k, top_p, seed, step, unfinished=None, eos=None, pad=None, row_seeds=None, return_logprob=False):
    """One sampled token per row of fp32/bf16 logits [rows, V]: temperature -> top-k (0 = off) -> top-p -> draw (csrc/sample.hip).
    seed: uint32 (row r uses seed + row_seeds[r] when row_seeds, an int32 device tensor [rows], is given); step: int, or an int32 device
    tensor of one element (read by the kernel).  unfinished: optional bool [rows], updated in place: finished rows get pad, a row that draws
    eos is finished.  Returns int64 [rows]; with return_logprob=True (tokens, logprob): float32 [rows], each draw's log-probability under
    the distribution it was drawn from (after temperature, top-k and top-p, renormalised), 0 for finished rows and for top_k = 1."""
    check_sampling(temperature, top_k, top_p)
    rows, V = logits.shape
    out = torch.empty(rows, device=logits.device, dtype=torch.int64)
    step_dev = None
    if torch.is_tensor(step):
        assert step.dtype == torch.int32 and step.numel() == 1 and step.is_cuda
        step_dev, step = step, 0
    if unfinished is not None:
        assert unfinished.dtype == torch.bool and unfinished.shape == (rows,) and unfinished.is_contiguous()
    if row_seeds is not None:
        assert row_seeds.dtype == torch.int32 and row_seeds.shape == (rows,) and row_seeds.is_contiguous()
    eos = -1 if eos is None else int(eos)
    pad = (eos if eos >= 0 else 0) if pad is None else int(pad)
    lp = torch.empty(rows, device=logits.device, dtype=torch.float32) if return_logprob else None
    L.check(L.load().avllm_sample_rows_scored(L.ptr(logits), _ld(logits), rows, V, float(temperature), int(top_k), float(top_p),
                                              int(seed) & 0xFFFFFFFF, L.ptr(row_seeds), int(step), L.ptr(step_dev), L.ptr(unfinished),
                                              eos, pad, L.ptr(out), L.ptr(lp), L.dt_of(logits), L.stream_ptr()))
    return (out, lp) if return_logprob else out


LOGITS_PROCESS_MAX_HISTORY = 1024


def check_logits_processors(repetition_penalty, no_repeat_ngram_size, min_new_tokens):
    """The argument rules of HF's RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor / MinNewTokensLengthLogitsProcessor
    (no_repeat_ngram_size = 0 turns the n-gram ban off, as in GenerationConfig).  Returns True when any of the three is on."""
    p = repetition_penalty
    if isinstance(p, bool) or not isinstance(p, numbers.Real) or not (0.0 < float(p) < float("inf")):
        raise ValueError(f"repetition_penalty must be a strictly positive float, got {p!r}")
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0:
            raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
    return float(p) != 1.0 or no_repeat_ngram_size > 0 or min_new_tokens > 0


LOGITS_BIAS_MAX_SEQUENCES, LOGITS_BIAS_MAX_SEQUENCE_LENGTH = 4096, 16      # AVLLM_LOGITS_MAX_SEQUENCES / _SEQUENCE_LEN of include/avllm.h

# Prepared device tables of logits_process (built by logits_bias_tables).  SequenceTable: tokens int32 [n, 16] (-1 padded), lengths int32 [n],
# values f32 [n] (None for bad words), entries grouped by last token; TokenTable: ids int32 [n], distinct and ascending.
SequenceTable = collections.namedtuple("SequenceTable", "tokens lengths values n max_len vocab")
TokenTable = collections.namedtuple("TokenTable", "ids n vocab")
# generate()'s keyword -> (table type, {field of avllm_logits_proc_desc: attribute of the table})
_TABLE_FIELDS = {
    "sequence_bias": (SequenceTable, dict(bias_tokens="tokens", bias_lengths="lengths", bias_values="values", n_bias="n", bias_max_len="max_len")),
    "bad_words_ids": (SequenceTable, dict(bad_tokens="tokens", bad_lengths="lengths", n_bad="n", bad_max_len="max_len")),
    "suppress_tokens": (TokenTable, dict(suppress="ids", n_suppress="n")),
    "begin_suppress_tokens": (TokenTable, dict(begin_suppress="ids", n_begin_suppress="n")),
}


def _token_ids(name, ids, vocab):
    """A list of token ids: non-negative integers below the vocabulary size (when it is known)."""
    if hasattr(ids, "tolist"):
        ids = ids.tolist()
    if isinstance(ids, (str, bytes, dict)) or not hasattr(ids, "__iter__"):
        raise ValueError(f"{name} must be a list of token ids, got {ids!r}")
    ids = list(ids)
    for t in ids:
        if isinstance(t, bool) or not isinstance(t, numbers.Integral) or t < 0:
            raise ValueError(f"{name} must hold non-negative integers, got {t!r}")
        if vocab is not None and t >= vocab:
            raise ValueError(f"{name}: token id {t} is outside the vocabulary of {vocab} entries")
    return [int(t) for t in ids]


def _sequences(name, seqs):
    if len(seqs) > LOGITS_BIAS_MAX_SEQUENCES:
        raise ValueError(f"{name} has {len(seqs)} sequences: at most LOGITS_BIAS_MAX_SEQUENCES = {LOGITS_BIAS_MAX_SEQUENCES} are supported")
    for q in seqs:
        if len(q) == 0:
            raise ValueError(f"{name} has an empty sequence")
        if len(q) > LOGITS_BIAS_MAX_SEQUENCE_LENGTH:
            raise ValueError(f"{name} has a sequence of {len(q)} tokens: at most LOGITS_BIAS_MAX_SEQUENCE_LENGTH = "
                             f"{LOGITS_BIAS_MAX_SEQUENCE_LENGTH} are supported")
    return seqs


def _normalise_logits_bias(sequence_bias, bad_words_ids, suppress_tokens, begin_suppress_tokens, vocab, eos):
    """The four arguments in one form each, or None where the processor is off: {tuple of ids: float} in HF's dict order, a list of distinct
    tuples ([eos] dropped), two ascending lists of distinct ids."""
    sb = bw = None
    if sequence_bias is not None:
        if isinstance(sequence_bias, dict):
            if any(not isinstance(k, tuple) for k in sequence_bias):
                raise ValueError(f"sequence_bias has to be a dict with tuples of token ids as keys, got {sequence_bias!r}")
            items = list(sequence_bias.items())
        elif isinstance(sequence_bias, (list, tuple)):
            if any(not isinstance(e, (list, tuple)) or len(e) != 2 or not isinstance(e[0], (list, tuple)) for e in sequence_bias):
                raise ValueError(f"sequence_bias has to be a list of [token ids, bias] pairs, got {sequence_bias!r}")
            items = [(tuple(e[0]), e[1]) for e in sequence_bias]
        else:
            raise ValueError(f"sequence_bias has to be a non-empty dict or list of [token ids, bias] pairs, got {sequence_bias!r}")
        if not items:
            raise ValueError("sequence_bias has to be non-empty")
        sb = {}
        for k, b in items:
            if isinstance(b, bool) or not isinstance(b, (float, np.floating)) or not math.isfinite(b):
                raise ValueError(f"sequence_bias: the bias of {k!r} must be a finite float, got {b!r}")
            sb[tuple(_token_ids("sequence_bias", k, vocab))] = float(b)
        _sequences("sequence_bias", list(sb))
    if bad_words_ids is not None:
        if not isinstance(bad_words_ids, (list, tuple)) or len(bad_words_ids) == 0:
            raise ValueError(f"bad_words_ids has to be a non-empty list, got {bad_words_ids!r}")
        if any(not isinstance(w, (list, tuple)) for w in bad_words_ids):
            raise ValueError(f"bad_words_ids has to be a list of lists of token ids, got {bad_words_ids!r}")
        bw = [tuple(_token_ids("bad_words_ids", w, vocab)) for w in bad_words_ids]
        bw = list(dict.fromkeys(w for w in bw if eos is None or w != (int(eos),)))         # HF's constructor drops [eos]
        if not bw:
            raise ValueError("bad_words_ids holds nothing but [eos], which HF drops: no sequence is left to ban")
        _sequences("bad_words_ids", bw)
    st = None if suppress_tokens is None else sorted(set(_token_ids("suppress_tokens", suppress_tokens, vocab)))
    bs = None if begin_suppress_tokens is None else sorted(set(_token_ids("begin_suppress_tokens", begin_suppress_tokens, vocab)))
    return sb, bw, st or None, bs or None


def check_logits_bias(sequence_bias=None, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, vocab=None, eos=None):
    """The argument rules of HF's SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor / SuppressTokensLogitsProcessor /
    SuppressTokensAtBeginLogitsProcessor and this library's capacities (LOGITS_BIAS_MAX_SEQUENCES sequences of at most
    LOGITS_BIAS_MAX_SEQUENCE_LENGTH tokens per table; suppress lists of any length): ValueError on token ids that are not non-negative
    integers (below `vocab` when given), empty sequences, biases that are not finite floats.  sequence_bias: {tuple of ids: float} or
    [[ids, float], ...]; bad_words_ids: [[ids], ...] ([eos] entries are dropped as HF drops them).  Returns True when any of the four is on."""
    return any(t is not None for t in _normalise_logits_bias(sequence_bias, bad_words_ids, suppress_tokens, begin_suppress_tokens, vocab, eos))


def logits_bias_tables(sequence_bias=None, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, *, vocab, eos=None,
                       device="cuda"):
    """The device tables logits_process takes under the same four names, as a dict to splat into it (empty when all four are off); built once
    per generate() call.  vocab: the width V of the score rows; eos: the model's EOS id or None."""
    sb, bw, st, bs = _normalise_logits_bias(sequence_bias, bad_words_ids, suppress_tokens, begin_suppress_tokens, int(vocab), eos)

    def seq_table(seqs, values):
        tok = np.full((len(seqs), LOGITS_BIAS_MAX_SEQUENCE_LENGTH), -1, dtype=np.int32)
        for i, q in enumerate(seqs):
            tok[i, :len(q)] = q
        ln = np.array([len(q) for q in seqs], dtype=np.int32)
        dev = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
        return SequenceTable(dev(tok), dev(ln), None if values is None else dev(np.array(values, dtype=np.float32)), len(seqs), int(ln.max()),
                             int(vocab))

    out = {}
    if sb is not None:
        # one fp32 total per last token, accumulated as HF does: the length-1 entry, then the longer sequences in the dict's order
        keys = sorted(sb, key=lambda q: (q[-1], len(q) != 1))                              # stable: dict order inside a group
        out["sequence_bias"] = seq_table(keys, [sb[q] for q in keys])
    if bw is not None:
        out["bad_words_ids"] = seq_table(bw, None)
    for name, ids in (("suppress_tokens", st), ("begin_suppress_tokens", bs)):
        if ids is not None:
            out[name] = TokenTable(torch.tensor(ids, dtype=torch.int32).to(device), len(ids), int(vocab))
    return out


def logits_process(scores, history, cur, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, eos=None, log_softmax=False,
                   append=None, *, sequence_bias=None, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None):
    """HF's logits processors IN PLACE on scores [rows, V] (f32 or bf16, row stride free) before argmax_rows / sample_rows /
    beam_topk(logprobs=True) (csrc/logits_process.hip), in GenerationMixin._get_logits_processor's order: sequence bias, repetition penalty,
    no-repeat n-gram, bad words, min-new-tokens, suppress, begin-suppress.  history: int64 [rows, ld] on
    the device, row r's first `cur` entries are its generated tokens; cur: int, or an int32 device tensor of one element (read by the
    kernel; then ld <= LOGITS_PROCESS_MAX_HISTORY).  eos: the model's EOS id or None (min_new_tokens then does nothing).  log_softmax (f32
    only): the row is first replaced by its log-softmax: HF's beam search runs the processors on log-probabilities.  append: optional int64
    [rows], stored at history[:, cur-1] before the history is read.  sequence_bias / bad_words_ids / suppress_tokens /
    begin_suppress_tokens: prepared device tables (logits_bias_tables(...), built for V = scores.shape[1]) or None.  With tables only of
    single-token entries and the three older processors and append off, history may be None and cur has no limit.  Returns scores."""
    check_logits_processors(repetition_penalty, no_repeat_ngram_size, min_new_tokens)
    if scores.dim() != 2 or not scores.is_cuda or scores.stride(1) != 1:
        raise ValueError("logits_process: scores must be a 2-d device tensor with unit column stride")
    rows, V = scores.shape
    cur_dev = None
    if torch.is_tensor(cur):
        assert cur.dtype == torch.int32 and cur.numel() == 1 and cur.is_cuda
        cur_dev, cur = cur, 0
    hptr, ldh = None, 0                            # no history: the library refuses when something needs it
    if history is not None:
        if history.dtype != torch.int64 or history.dim() != 2 or history.shape[0] != rows or not history.is_cuda or \
                (history.shape[1] > 1 and history.stride(1) != 1):
            raise ValueError(f"logits_process: history must be an int64 device tensor [{rows}, ld] with unit column stride")
        ldh = history.stride(0) if rows > 1 and history.shape[1] > 0 else history.shape[1]
        if cur_dev is None and int(cur) > history.shape[1]:
            raise ValueError(f"logits_process: history length {cur} > the {history.shape[1]} columns of history")
        hptr = L.ptr(history) if history.numel() else None
    if append is not None:
        assert append.dtype == torch.int64 and append.shape == (rows,) and append.is_contiguous() and append.is_cuda
    d = L.LogitsProcDesc(scores=L.ptr(scores), ld=_ld(scores), rows=rows, V=V, dtype=L.dt_of(scores), history=hptr, ldh=ldh, append=L.ptr(append),
                         cur=int(cur), cur_dev=L.ptr(cur_dev), repetition_penalty=float(repetition_penalty),
                         no_repeat_ngram_size=int(no_repeat_ngram_size), min_new_tokens=int(min_new_tokens), eos=-1 if eos is None else int(eos),
                         log_softmax=int(bool(log_softmax)))
    for (name, (kind, fields)), t in zip(_TABLE_FIELDS.items(), (sequence_bias, bad_words_ids, suppress_tokens, begin_suppress_tokens)):
        if t is None:
            continue
        if not isinstance(t, kind):
            raise ValueError(f"logits_process: {name} must be a prepared {kind.__name__} (ops.logits_bias_tables), got {type(t).__name__}")
        if t.vocab != V:
            raise ValueError(f"logits_process: the {name} table was built for a vocabulary of {t.vocab}, the scores have {V} columns")
        for field, attr in fields.items():
            v = getattr(t, attr)
            setattr(d, field, L.ptr(v) if torch.is_tensor(v) else v)
    L.check(L.load().avllm_logits_process_ex(C.byref(d), L.stream_ptr()))
    return scores


BEAM_MAX_BEAMS, BEAM_MAX_K = 16, 32


def beam_topk(logits, beam_scores, num_beams, k, logprobs=False):
    """Beam-search candidates (csrc/beam.hip): for each batch item b, the k best of beam_scores[b*nb + j] + log_softmax(logits[b*nb + j])[v]
    over all nb*V pairs, sorted descending, equal scores by the lower flat index j*V + v first.  logits: f32 [B*nb, V] (row stride free);
    beam_scores: f32 [B*nb].  logprobs=True: the rows are log-probabilities already (logits_process(..., log_softmax=True)) and are added
    to beam_scores as they are.  Returns (scores f32 [B, k], beams int32 [B, k], tokens int64 [B, k])."""
    nb, k = int(num_beams), int(k)
    if not 1 <= nb <= BEAM_MAX_BEAMS:
        raise ValueError(f"num_beams must be in [1, {BEAM_MAX_BEAMS}], got {num_beams}")
    if not 1 <= k <= BEAM_MAX_K:
        raise ValueError(f"k must be in [1, {BEAM_MAX_K}], got {k}")
    if logits.dtype != torch.float32 or logits.dim() != 2 or not logits.is_cuda:
        raise ValueError("beam_topk: logits must be a 2-d float32 device tensor")
    rows, V = logits.shape
    if rows % nb:
        raise ValueError(f"beam_topk: {rows} logits rows are not a multiple of num_beams = {nb}")
    if k > nb * V:
        raise ValueError(f"beam_topk: k = {k} > num_beams * V = {nb * V}")
    if beam_scores.dtype != torch.float32 or beam_scores.numel() != rows or not beam_scores.is_cuda:
        raise ValueError(f"beam_topk: beam_scores must be float32 [{rows}] on the device")
    beam_scores = beam_scores.contiguous()
    B = rows // nb
    lib = L.load()
    ws = torch.empty(lib.avllm_beam_topk_workspace_bytes(rows, V, k), device=logits.device, dtype=torch.uint8)
    scores = torch.empty(B, k, device=logits.device, dtype=torch.float32)
    beams = torch.empty(B, k, device=logits.device, dtype=torch.int32)
    tokens = torch.empty(B, k, device=logits.device, dtype=torch.int64)
    fn = lib.avllm_beam_topk_logprobs if logprobs else lib.avllm_beam_topk
    L.check(fn(L.ptr(logits), _ld(logits), B, nb, V, L.ptr(beam_scores), k, L.ptr(scores), L.ptr(beams), L.ptr(tokens), L.ptr(ws), ws.numel(),
               L.stream_ptr()))
    return scores, beams, tokens


def kv_gather_rows(k_src, v_src, k_dst, v_dst, parent, t0, t1):
    """dst[l, r, t, :] = src[l, parent[r], t, :] for t in [t0, t1), on K and V (csrc/beam.hip).  Caches: contiguous [layers, rows, T, dkv],
    f32 or bf16; src may have fewer rows and another T than dst; src is dst gives an in-place reorder (correct for any parent map).
    parent: int32 [dst rows] on the device; entries outside [0, src rows) leave that row untouched."""
    for t in (k_src, v_src, k_dst, v_dst):
        if t.dim() != 4 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("kv_gather_rows: caches must be contiguous 4-d device tensors [layers, rows, T, dkv]")
    if k_src.shape != v_src.shape or k_dst.shape != v_dst.shape:
        raise ValueError("kv_gather_rows: K and V caches must have equal shapes")
    if len({k_src.dtype, v_src.dtype, k_dst.dtype, v_dst.dtype}) != 1:
        raise ValueError("kv_gather_rows: all caches must have one dtype")
    Ls, Rs, Ts, D = k_src.shape
    Ld, Rd, Td, Dd = k_dst.shape
    if Ls != Ld or D != Dd:
        raise ValueError(f"kv_gather_rows: src {tuple(k_src.shape)} and dst {tuple(k_dst.shape)} differ in layers or width")
    if (k_src.data_ptr() == k_dst.data_ptr()) != (v_src.data_ptr() == v_dst.data_ptr()):
        raise ValueError("kv_gather_rows: K and V must both be in place or both out of place")
    if parent.dtype != torch.int32 or parent.shape != (Rd,) or not parent.is_contiguous() or not parent.is_cuda:
        raise ValueError(f"kv_gather_rows: parent must be a contiguous int32 device tensor [{Rd}]")
    t0, t1 = int(t0), int(t1)
    if not 0 <= t0 <= t1 <= min(Ts, Td):
        raise ValueError(f"kv_gather_rows: positions [{t0}, {t1}) outside the caches (T = {Ts}, {Td})")
    L.check(L.load().avllm_kv_gather_rows(L.ptr(k_src), L.ptr(v_src), Rs, Ts, L.ptr(k_dst), L.ptr(v_dst), Rd, Td, Ls, D, L.ptr(parent),
                                          t0, t1, L.dt_of(k_dst), L.stream_ptr()))


def embedding(table, ids):
    ids = ids.contiguous()
    out = torch.empty(*ids.shape, table.shape[1], device=table.device, dtype=table.dtype)
    L.check(L.load().avllm_embedding(L.ptr(table), L.ptr(ids), L.ptr(out), ids.numel(), table.shape[1], L.dt_of(table), L.stream_ptr()))
    return out


def cast(x, dtype):
    if x.dtype == dtype:
        return x
    x = x.contiguous()
    out = torch.empty_like(x, dtype=dtype)
    if x.numel():
        L.check(L.load().avllm_cast(L.ptr(x), L.dt_of(x), L.ptr(out), L.dt_of(out), x.numel(), L.stream_ptr()))
    return out


def act_residual(x, act, r=None):
    """act(x) + r elementwise (avllm_act_residual)."""
    x = x.contiguous()
    y = torch.empty_like(x)
    L.check(L.load().avllm_act_residual(L.ptr(x), L.ptr(r.contiguous()) if r is not None else None, L.ptr(y), x.numel(), act, L.dt_of(x), L.stream_ptr()))
    return y


def conv1d_k3(x, w2d, bias, stride=1):
    """nn.Conv1d(kernel_size=3, padding=1, stride) on token-major x [B,T,C]: avllm_im2col_k3 + avllm_gemm.  w2d = weight [out, C, 3] reshaped to
    [out, kw*C + c] (permute(0, 2, 1)), zero-padded along K to a multiple of 64 by the caller when 3C is not one."""
    B, T, Cc = x.shape
    To = (T - 1) // stride + 1
    K = w2d.shape[1]
    x = x.contiguous()
    cols = torch.empty(B * To, 3 * Cc, device=x.device, dtype=x.dtype) if K == 3 * Cc else torch.zeros(B * To, K, device=x.device, dtype=x.dtype)
    if K == 3 * Cc:
        L.check(L.load().avllm_im2col_k3(L.ptr(x), L.ptr(cols), B, T, Cc, stride, L.dt_of(x), L.stream_ptr()))
    else:                                                       # padded K: im2col into a dense scratch, then one strided copy into the padded rows
        dense = torch.empty(B * To, 3 * Cc, device=x.device, dtype=x.dtype)
        L.check(L.load().avllm_im2col_k3(L.ptr(x), L.ptr(dense), B, T, Cc, stride, L.dt_of(x), L.stream_ptr()))
        cols[:, : 3 * Cc] = dense
    return gemm(cols, w2d, bias=bias).view(B, To, -1)


def groupnorm_tokens(x, w, b, groups, eps=1e-5, act=L.ACT_NONE):
    """nn.GroupNorm(groups, C) of the [B,C,T] view of x [B,T,C] (+ activation)."""
    B, T, Cc = x.shape
    x = x.contiguous()
    y = torch.empty_like(x)
    L.check(L.load().avllm_groupnorm_tokens(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), B, T, Cc, groups, eps, act, L.dt_of(x), L.stream_ptr()))
    return y


def mha_self(x, in_w, in_b, out_w, out_b, heads):
    """nn.MultiheadAttention(batch_first=True)(x, x, x) in eval mode: packed in-projection (avllm_gemm), softmax(QK^T / sqrt(hd)) V per head
    (avllm_attention_fwd; head dims up to 512 go to the scalar kernel), out-projection.  x [B,T,E]."""
    B, T, E = x.shape
    qkv = gemm(x.reshape(B * T, E), in_w, bias=in_b)
    o, _ = attention_fwd(qkv, B, T, heads, E // heads, causal=False, want_lse=False)
    return gemm(o, out_w, bias=out_b).view(B, T, E)


def fuse_pool(a, v, prompt_emb, L_, S_out, fusion_scale, D, B):
    """See avllm_fuse_pool in include/avllm.h.  a [B,Ta,D] | None, v [B,Tv,D] | None, prompt_emb [B,P,D] | None."""
    ref = a if a is not None else v
    out = torch.empty(B, S_out, D, device=ref.device, dtype=ref.dtype)
    Ta = a.shape[1] if a is not None else 0
    Tv = v.shape[1] if v is not None else 0
    P = prompt_emb.shape[1] if prompt_emb is not None else 0
    L.check(L.load().avllm_fuse_pool(L.ptr(a), Ta, L.ptr(v), Tv, L.ptr(prompt_emb), P, L.ptr(out), B, L_, S_out, D, fusion_scale,
                                     L.dt_of(ref), L.stream_ptr()))
    return out


def fuse_pool_bwd(dx, Ta, Tv, P, L_, fusion_scale, want_a=True, want_v=True, da=None, dv=None):
    """The adjoint of fuse_pool (avllm_fuse_pool_bwd): dx [B,S_out,D] -> (da [B,Ta,D] | None, dv [B,Tv,D] | None).  Ta / Tv are the forward's row
    counts (0 = that input was absent); want_a / want_v choose the outputs; da / dv: preallocated outputs (static buffers of a captured step)."""
    dx = dx.contiguous()
    B, S_out, D = dx.shape
    if want_a and Ta and da is None:
        da = torch.empty(B, Ta, D, device=dx.device, dtype=dx.dtype)
    if want_v and Tv and dv is None:
        dv = torch.empty(B, Tv, D, device=dx.device, dtype=dx.dtype)
    da = da if want_a and Ta else None
    dv = dv if want_v and Tv else None
    L.check(L.load().avllm_fuse_pool_bwd(L.ptr(dx), L.ptr(da), Ta, L.ptr(dv), Tv, P, B, L_, S_out, D, fusion_scale, L.dt_of(dx), L.stream_ptr()))
    return da, dv


def _check_modes(name, mode, B, device):
    if not isinstance(mode, torch.Tensor) or mode.dtype != torch.int32 or mode.dim() != 1 or mode.shape[0] != B or not mode.is_contiguous():
        raise ValueError(f"{name}: mode must be a contiguous int32 tensor [{B}], got "
                         f"{(tuple(mode.shape), mode.dtype) if isinstance(mode, torch.Tensor) else type(mode).__name__}")
    if mode.device != device:
        raise ValueError(f"{name}: mode lives on {mode.device}, the inputs on {device}")


def fuse_pool_rows(a, v, prompt_emb, mode, L_, S_out, fusion_scale, D, B):
    """fuse_pool with one mode per clip (avllm_fuse_pool_rows): mode int32 [B] on the device, 0 both | 1 audio only | 2 video only.
    a [B,Ta,D] and v [B,Tv,D] are both required; prompt_emb [B,P,D] | None.  The stream a row does not use is not read for that row."""
    if a is None or v is None:
        raise ValueError(f"fuse_pool_rows: modes need both inputs ({'a' if a is None else 'v'} is None); a call on one stream is fuse_pool")
    if a.dtype != v.dtype or a.shape[0] != B or v.shape[0] != B or a.shape[2] != D or v.shape[2] != D:
        raise ValueError(f"fuse_pool_rows: a {tuple(a.shape)} {a.dtype} and v {tuple(v.shape)} {v.dtype} do not match B={B}, D={D}")
    _check_modes("fuse_pool_rows", mode, B, a.device)
    a, v = a.contiguous(), v.contiguous()
    out = torch.empty(B, S_out, D, device=a.device, dtype=a.dtype)
    P = prompt_emb.shape[1] if prompt_emb is not None else 0
    L.check(L.load().avllm_fuse_pool_rows(L.ptr(a), a.shape[1], L.ptr(v), v.shape[1], L.ptr(prompt_emb), P, L.ptr(mode), L.ptr(out), B, L_, S_out, D,
                                          fusion_scale, L.dt_of(a), L.stream_ptr()))
    return out


def fuse_pool_rows_bwd(dx, mode, Ta, Tv, P, L_, fusion_scale, da=None, dv=None):
    """The adjoint of fuse_pool_rows (avllm_fuse_pool_rows_bwd): dx [B,S_out,D] -> (da [B,Ta,D], dv [B,Tv,D]), both overwritten; a row's unused
    stream gets exact zeros.  da / dv: preallocated outputs (static buffers of a captured step)."""
    dx = dx.contiguous()
    B, S_out, D = dx.shape
    if Ta <= 0 or Tv <= 0:
        raise ValueError(f"fuse_pool_rows_bwd: modes need both inputs (Ta={Ta}, Tv={Tv}); the adjoint of a call on one stream is fuse_pool_bwd")
    _check_modes("fuse_pool_rows_bwd", mode, B, dx.device)
    if da is None:
        da = torch.empty(B, Ta, D, device=dx.device, dtype=dx.dtype)
    if dv is None:
        dv = torch.empty(B, Tv, D, device=dx.device, dtype=dx.dtype)
    for nm, t, T in (("da", da, Ta), ("dv", dv, Tv)):
        if tuple(t.shape) != (B, T, D) or t.dtype != dx.dtype or not t.is_contiguous():
            raise ValueError(f"fuse_pool_rows_bwd: {nm} {tuple(t.shape)} {t.dtype} is not a contiguous [{B}, {T}, {D}] {dx.dtype}")
    L.check(L.load().avllm_fuse_pool_rows_bwd(L.ptr(dx), L.ptr(da), Ta, L.ptr(dv), Tv, P, L.ptr(mode), B, L_, S_out, D, fusion_scale, L.dt_of(dx),
                                              L.stream_ptr()))
    return da, dv


def modality_draw(B, p_drop_audio, p_drop_video, seed=0, seed_dev=None, mode_in=None, out=None, device="cuda"):
    """Draws one mode per clip on the device (avllm_modality_draw; the rule is in include/avllm.h): int32 [B], 2 with probability p_drop_audio
    (audio dropped), 1 with p_drop_video, else 0.  mode_in int32 [B] | None: entries 1 / 2 are kept.  seed_dev: the address of a device uint32
    (or a one-element int32 device tensor) added to seed at run time; out: a preallocated result (static buffer of a captured step)."""
    pa, pv = float(p_drop_audio), float(p_drop_video)
    if not (0.0 <= pa <= 1.0 and 0.0 <= pv <= 1.0 and pa + pv <= 1.0):
        raise ValueError(f"modality_draw: p_drop_audio={pa} and p_drop_video={pv} must lie in [0, 1] with a sum of at most 1")
    if out is None:
        out = torch.empty(B, dtype=torch.int32, device=mode_in.device if mode_in is not None else device)
    _check_modes("modality_draw (out)", out, B, out.device)
    if mode_in is not None:
        _check_modes("modality_draw (mode_in)", mode_in, B, out.device)
    if isinstance(seed_dev, torch.Tensor):
        if seed_dev.numel() != 1 or seed_dev.element_size() != 4:
            raise ValueError(f"modality_draw: seed_dev must hold one 32-bit word, got {tuple(seed_dev.shape)} {seed_dev.dtype}")
        seed_dev = L.ptr(seed_dev)
    L.check(L.load().avllm_modality_draw(L.ptr(mode_in), L.ptr(out), B, pa, pv, int(seed) & 0xFFFFFFFF, seed_dev, L.stream_ptr()))
    return out


def gemm_wgrad(dY, X, alpha=1.0, dW=None, db=None, want_db=True):
    """dW [N,K] (fp32) = alpha * dY^T . X and db [N] (fp32) = alpha * column sums of dY, for dY [M,N], X [M,K] (avllm_gemm_wgrad: no atomics)."""
    M, N = dY.shape
    K = X.shape[1]
    if X.shape[0] != M or X.dtype != dY.dtype:
        raise ValueError(f"gemm_wgrad: dY {tuple(dY.shape)} {dY.dtype} and X {tuple(X.shape)} {X.dtype} do not match")
    if dW is None:
        dW = torch.empty(N, K, device=dY.device, dtype=torch.float32)
    if db is None and want_db:
        db = torch.empty(N, device=dY.device, dtype=torch.float32)
    L.check(L.load().avllm_gemm_wgrad(L.ptr(dY), _ld(dY), L.ptr(X), _ld(X), M, N, K, L.ptr(dW), _ld(dW), L.ptr(db), alpha, L.dt_of(dY),
                                      L.stream_ptr()))
    return dW, db


def gemm_wgrad_acc(dY, X, dW, db=None, alpha=1.0):
    """dW [N,K] (fp32) += alpha * dY^T . X and db [N] (fp32, optional) += alpha * column sums of dY (avllm_gemm_wgrad_acc: the prior value is
    read once and added once, no atomics)."""
    M, N = dY.shape
    K = X.shape[1]
    if X.shape[0] != M or X.dtype != dY.dtype:
        raise ValueError(f"gemm_wgrad_acc: dY {tuple(dY.shape)} {dY.dtype} and X {tuple(X.shape)} {X.dtype} do not match")
    if dW.dtype != torch.float32 or tuple(dW.shape) != (N, K) or (db is not None and (db.dtype != torch.float32 or db.numel() != N)):
        raise ValueError(f"gemm_wgrad_acc: dW must be fp32 [{N},{K}] and db fp32 [{N}]")
    L.check(L.load().avllm_gemm_wgrad_acc(L.ptr(dY), _ld(dY), L.ptr(X), _ld(X), M, N, K, L.ptr(dW), _ld(dW), L.ptr(db), alpha, L.dt_of(dY),
                                          L.stream_ptr()))
    return dW, db


def grad_sumsq_multi(gs, out, partials):
    """out = sum over the buffers `gs` (in order) of sum g^2, in a fixed order (avllm_grad_sumsq_det_multi)."""
    n = len(gs)
    ptrs = (L.vp * n)(*[L.ptr(g) for g in gs])
    lens = (L.i64 * n)(*[g.numel() for g in gs])
    L.check(L.load().avllm_grad_sumsq_det_multi(ptrs, lens, n, L.ptr(partials), partials.numel(), L.ptr(out), L.stream_ptr()))


def _grad_div_ptr(grad_div, who):
    if not (torch.is_tensor(grad_div) and grad_div.dtype == torch.float32 and grad_div.numel() == 1):
        raise ValueError(f"{who}: grad_div must be a device tensor of one float32")
    return L.ptr(grad_div)


def adamw_step_multi(segs, lr, step, sumsq=None, max_norm=0.0, beta1=0.9, beta2=0.95, eps=1e-8, prescale=1.0, guard=None, skipped=None, state=None,
                     grad_div=None):
    """One AdamW step over several flat fp32 buffers under one guard decision (avllm_adamw_step_multi).  segs: (p, g, m, v, weight_decay) each.
    grad_div: a device float; the prescale is then 1 / grad_div, read on the device (avllm_adamw_step_multi_dev; `prescale` is not used)."""
    arr = (L.AdamwSeg * len(segs))()
    for a, (p, g, m, v, wd) in zip(arr, segs):
        a.p, a.g, a.m, a.v, a.n, a.weight_decay = L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), wd
    if grad_div is not None:
        L.check(L.load().avllm_adamw_step_multi_dev(arr, len(segs), lr, beta1, beta2, eps, step, L.ptr(sumsq), max_norm,
                                                    _grad_div_ptr(grad_div, "adamw_step_multi"), L.ptr(guard), L.ptr(skipped), L.ptr(state),
                                                    L.stream_ptr()))
        return
    L.check(L.load().avllm_adamw_step_multi(arr, len(segs), lr, beta1, beta2, eps, step, L.ptr(sumsq), max_norm, prescale, L.ptr(guard),
                                            L.ptr(skipped), L.ptr(state), L.stream_ptr()))


def grad_sumsq(g, out, partials=None):
    """out += sum g^2 (float atomics), or -- with a `partials` scratch tensor (float32, <= 1024 used) -- out = sum g^2 in a fixed order."""
    if partials is not None:
        L.check(L.load().avllm_grad_sumsq_det(L.ptr(g), g.numel(), L.ptr(partials), partials.numel(), L.ptr(out), L.stream_ptr()))
        return
    L.check(L.load().avllm_grad_sumsq(L.ptr(g), g.numel(), L.ptr(out), L.stream_ptr()))


def adamw_step(p, g, m, v, lr, step, sumsq=None, max_norm=0.0, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.01, prescale=1.0, guard=None,
               skipped=None, state=None, grad_div=None):
    """guard: device float (e.g. the step's loss_sum); a non-finite guard or sumsq makes the launch a no-op and bumps `skipped`.
    state: device avllm_step_state (uint8 tensor): lr and Adam's bias corrections are read from it instead of `lr` / `step`.
    grad_div: a device float; the prescale is then 1 / grad_div, read on the device (avllm_adamw_step_dev; `prescale` is not used)."""
    if grad_div is not None:
        L.check(L.load().avllm_adamw_step_dev(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), lr, beta1, beta2, eps, wd, step, L.ptr(sumsq),
                                              max_norm, _grad_div_ptr(grad_div, "adamw_step"), L.ptr(guard), L.ptr(skipped), L.ptr(state),
                                              L.stream_ptr()))
        return
    L.check(L.load().avllm_adamw_step(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), lr, beta1, beta2, eps, wd, step,
                                      L.ptr(sumsq), max_norm, prescale, L.ptr(guard), L.ptr(skipped), L.ptr(state), L.stream_ptr()))


def lora_dx_masked(Ts, ATs, seeds, r, p, R=None, out=None, seed_dev=None):
    """out = R + sum_j mask_j o (T_j . A_j)/(1-p): the adapters' input gradient under LoRA dropout in one pass (avllm_lora_dx_masked).
    Ts[j] [M,>=32] (zeros past r), ATs[j] [N,>=32] padded transposed A images; out may be R."""
    n = len(Ts)
    M, N = Ts[0].shape[0], ATs[0].shape[0]
    if out is None:
        out = torch.empty(M, N, device=Ts[0].device, dtype=Ts[0].dtype)
    arr = lambda ty, vals: (ty * n)(*vals)
    L.check(L.load().avllm_lora_dx_masked(arr(L.vp, [L.ptr(t) for t in Ts]), arr(L.i64, [_ld(t) for t in Ts]), arr(L.vp, [L.ptr(t) for t in ATs]),
                                          arr(L.i64, [_ld(t) for t in ATs]), arr(C.c_uint32, [s & 0xFFFFFFFF for s in seeds]), n, r, L.ptr(R),
                                          _ld(R) if R is not None else 0, L.ptr(out), _ld(out), M, N, p, seed_dev, L.dt_of(out), L.stream_ptr()))
    return out


def lora_rank3(As, Bs, outs, r, alpha=1.0, seeds=None, p=0.0, shared=False, seed_dev=None):
    """Batched rank-side products of up to 3 adapters (avllm_lora_rank3): outs[j][M,64] = alpha * A_j . Bs[j][:r]^T, columns >= r zero.
    Bs[j] is the PADDED image [>= 16, K]: the kernel is not told r, reads 16 rows of every B and writes all 16 products, so rows r..15 must be
    zeros (avllm_lora_pack's layout); a true [r, K] tensor with r < 16 is an out-of-bounds read.  All 64 columns of every output are written.
    shared=True: every adapter reads As[0] (contiguous [M, K]) through its own dropout mask (seeds[j], p); seed_dev: pointer to a device uint32
    added to every seed."""
    n = len(Bs)
    arr = lambda ty, vals: (ty * n)(*vals)
    Aa = [As[0]] * n if shared else As
    L.check(L.load().avllm_lora_rank3(arr(L.vp, [L.ptr(t) for t in Aa]), arr(L.i64, [_ld(t) for t in Aa]), arr(L.i32, [t.shape[1] for t in Aa]),
                                      arr(L.vp, [L.ptr(t) for t in Bs]), arr(L.i64, [_ld(t) for t in Bs]), arr(L.vp, [L.ptr(t) for t in outs]),
                                      arr(L.i64, [_ld(t) for t in outs]), arr(C.c_uint32, [(s & 0xFFFFFFFF) for s in (seeds or [0] * n)]), n,
                                      Aa[0].shape[0], r, alpha, p, seed_dev, int(shared), L.dt_of(Aa[0]), L.stream_ptr()))
    return outs


def gemm_tn_multi(big, smalls, outs, r, alpha=1.0, seeds=None, p=0.0, shared=False, cols=None, seed_dev=None):
    """Batched LoRA-gradient reductions over tokens (avllm_gemm_tn_multi), ACCUMULATING into the fp32 outs.
    shared=True: outs[j][r, NB] += alpha * smalls[j]^T . dropout_j(big); shared=False: outs[j][ncol_j, r] += alpha * big[:, cols[j]]^T . smalls[j]
    with cols = [(col0, ncol), ...] tiling big's columns."""
    n = len(smalls)
    arr = lambda ty, vals: (ty * n)(*vals)
    c0 = arr(L.i32, [c[0] for c in cols]) if cols else None
    nc = arr(L.i32, [c[1] for c in cols]) if cols else None
    L.check(L.load().avllm_gemm_tn_multi(L.ptr(big), _ld(big), big.shape[1], arr(L.vp, [L.ptr(t) for t in smalls]), arr(L.i64, [_ld(t) for t in smalls]),
                                         arr(L.vp, [L.ptr(t) for t in outs]), arr(L.i64, [_ld(t) for t in outs]), c0, nc,
                                         arr(C.c_uint32, [(s & 0xFFFFFFFF) for s in (seeds or [0] * n)]), n, r, big.shape[0], alpha, p, seed_dev,
                                         int(shared), L.dt_of(big), L.stream_ptr()))
    return outs


def lora_merge_(W, A, B, scale):
    """In place W[n,k] <- round(W[n,k] + scale * sum_j B[n,j] A[j,k]) (avllm_lora_merge): the decode-time merge of one LoRA pair.
    W [N,K] f32 or bf16 with unit column stride (a row slice of a larger matrix is fine); A [r,K], B [N,r] contiguous fp32 masters."""
    if W.dim() != 2 or A.dim() != 2 or B.dim() != 2 or A.shape[1] != W.shape[1] or B.shape[0] != W.shape[0] or A.shape[0] != B.shape[1]:
        raise ValueError(f"lora_merge: shapes W {tuple(W.shape)}, A {tuple(A.shape)}, B {tuple(B.shape)} are not [N,K], [r,K], [N,r]")
    if W.dtype not in (torch.float32, torch.bfloat16) or A.dtype != torch.float32 or B.dtype != torch.float32:
        raise ValueError(f"lora_merge: W must be float32 or bfloat16 and A, B float32, got {W.dtype}, {A.dtype}, {B.dtype}")
    if W.stride(1) != 1 or not (A.is_contiguous() and B.is_contiguous()):
        raise ValueError("lora_merge: W needs unit column stride, A and B must be contiguous")
    N, K = W.shape
    L.check(L.load().avllm_lora_merge(L.ptr(W), W.stride(0), N, K, L.ptr(A), L.ptr(B), A.shape[0], float(scale), L.dt_of(W), L.stream_ptr()))
    return W


def mx_quantize(x, layout=0, q=None, s=None):
    """x [R,K] bf16/f32 -> (q uint8 [R,K] e4m3, scale image uint8 tensor): OCP-MX block scaling, 32 elements per E8M0 scale.
    layout 0 = activation side, 1 = weight side of avllm_gemm_f8; layout 2 = decode side: the scales are the exponent matrix uint8 [R, K/32]
    (E8M0 biased by 127) of dec_proj's fp8 weight form.  `q`: optional [R, K] uint8 output for the codes (the same for every layout; a column slice of a wider buffer passes its row stride); `s`: the
    scale image of an earlier call with the same shape and layout, rewritten in place (a weight that changed keeps its buffers)."""
    lib = L.load()
    R, K = x.shape
    if q is None:
        q = torch.empty(R, K, device=x.device, dtype=torch.uint8)
    if s is None:
        s = torch.zeros((R, K // 32) if layout == 2 else lib.avllm_mx_scale_bytes(R, K), device=x.device, dtype=torch.uint8)
    L.check(lib.avllm_mx_quantize(L.ptr(x), _ld(x), R, K, L.ptr(q), _ld(q), L.ptr(s), layout, L.dt_of(x), L.stream_ptr()))
    return q, s


def mx4_quantize(x, out=None):
    """x [R,K] bf16/f32 (K % 32 == 0) -> (codes uint8 [R, K/2], exponents uint8 [R, K/32]): OCP MXFP4 -- e2m1 elements, two per byte with
    element 2i in the low nibble, one E8M0 exponent (biased by 127) per 32 elements; the W4 / E8 of dec_proj's fp4 weight form.
    `out`: the (codes, exponents) pair of an earlier call with the same shape, rewritten in place."""
    R, K = x.shape
    if K % 32:
        raise ValueError(f"mx4_quantize: K={K} must be a multiple of 32")
    q, e = out if out is not None else (torch.empty(R, K // 2, device=x.device, dtype=torch.uint8),
                                        torch.empty(R, K // 32, device=x.device, dtype=torch.uint8))
    L.check(L.load().avllm_mx4_quantize(L.ptr(x), _ld(x), R, K, L.ptr(q), K // 2, L.ptr(e), L.dt_of(x), L.stream_ptr()))
    return q, e


def gemm_f8(Aq, As, Bq, Bs, out=None, bias=None, R=None, act=L.ACT_NONE, quantised_out=False, plan=False):
    """out[M,N] (bf16) = act(A.B^T + bias) + R on the block-scaled fp8 matrix pipe; (Aq, As) / (Bq, Bs) from mx_quantize(layout 0 / 1).
    quantised_out=True: returns (codes uint8 [M,N], scale image) = the e4m3 block-scaled result, quantised in the epilogue (no bf16 copy).
    plan=True: launches nothing and returns the kernel avllm_gemm_f8 would run this very call on: "fast" (the persistent 256x256 kernel) or
    "ref" (the reference-grade one; with quantised_out that is a call avllm_gemm_f8 refuses)."""
    M, K = Aq.shape
    N = Bq.shape[0]
    d = L.GemmF8Desc()
    d.A, d.SA, d.B, d.SB, d.bias = L.ptr(Aq), L.ptr(As), L.ptr(Bq), L.ptr(Bs), L.ptr(bias)
    d.lda, d.ldb = _ld(Aq), _ld(Bq)
    d.M, d.N, d.K, d.act = M, N, K, act
    if quantised_out:
        q = torch.empty(M, N, device=Aq.device, dtype=torch.uint8)
        sc = torch.zeros(L.load().avllm_mx_scale_bytes(M, N), device=Aq.device, dtype=torch.uint8)
        d.Cq, d.SCq, d.ldcq = L.ptr(q), L.ptr(sc), N
        if plan:
            return "fast" if L.load().avllm_gemm_f8_takes_fast(C.byref(d)) else "ref"
        L.check(L.load().avllm_gemm_f8(C.byref(d), L.stream_ptr()))
        return q, sc
    if out is None:
        out = torch.empty(M, N, device=Aq.device, dtype=torch.bfloat16)
    d.C, d.ldc = L.ptr(out), _ld(out)
    if R is not None:
        d.R, d.ldr = L.ptr(R), _ld(R)
    if plan:
        return "fast" if L.load().avllm_gemm_f8_takes_fast(C.byref(d)) else "ref"
    L.check(L.load().avllm_gemm_f8(C.byref(d), L.stream_ptr()))
    return out


def norm_mxq(x, w, b=None, eps=1e-5, want_y=False, want_rstd=False, q=None):
    """LayerNorm (b given) / RMSNorm (b None) of bf16 rows, block-scaled to e4m3 in the same pass (avllm_norm_mxq):
    -> (codes uint8 [rows, d], scale image, y bf16 | None, rstd | None).  `q`: optional [rows, d] uint8 output for the codes; its row stride is
    passed as ldq (a column slice of a wider buffer)."""
    rows, d = x.shape
    if q is None:
        q = torch.empty(rows, d, device=x.device, dtype=torch.uint8)
    sc = torch.zeros(L.load().avllm_mx_scale_bytes(rows, d), device=x.device, dtype=torch.uint8)
    y = torch.empty_like(x) if want_y else None
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32) if want_rstd else None
    L.check(L.load().avllm_norm_mxq(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(rstd), L.ptr(q), _ld(q), L.ptr(sc), rows, d, eps, L.stream_ptr()))
    return q, sc, y, rstd


def dec_proj(A, W, mode=0, norm_w=None, eps=1e-5, R=None, out=None, out_f32=False, rope=None, kc=None, vc=None, pos=0, pos_dev=None, dq=0, dkv=0, hd=0,
             lora_t=None, lora_b=None, lora_r=0, lora_scale=0.0, W8=None, E8=None, W4=None, bias=None, raw_qkv=False):
    """One projection of a decode token step (avllm_dec_proj): A [M<=16, K] bf16, W [rows, K] bf16.
    mode 0: out[M, rows] = rmsnorm?(A) . W^T (+ R);  mode 1: W = [gate; up], out[M, rows/2] = silu(gate) * up;
    mode 2: W = [q; k; v]: RoPE on q, k with `rope` [hd/2, 2]; q -> out[M, dq]; k, v -> kc / vc [M, Tmax, dkv] at row pos (+ *pos_dev);
    hd must be a power of two >= 32 (any other head dim raises ValueError).
    fp8 weight form: W8 = e4m3 codes uint8 [rows, K], E8 = exponents uint8 [rows, K/32] (mx_quantize(w, 2)); W may then be None.
    fp4 weight form: W4 = MXFP4 codes uint8 [rows, K/2], E8 = their exponents uint8 [rows, K/32] (mx4_quantize(w)); not together with W8.
    bias: bf16 [rows] in W's row order, added before adapters, residual and RoPE (modes 0 and 2).
    raw_qkv (mode 2): no rotation, no cache write; q, k and v all go to out[M, rows] in logical column order (a head norm follows: qk_norm_rope_)."""
    M, K = A.shape
    d = L.DecProjDesc()
    Wr = W4 if W4 is not None else (W8 if W8 is not None else W)
    d.A, d.lda, d.M, d.K, d.mode = L.ptr(A), _ld(A), M, K, mode
    d.W, d.ldw = L.ptr(W), _ld(Wr)
    if W8 is not None:
        d.W8, d.E8 = L.ptr(W8), L.ptr(E8)
    if W4 is not None:
        d.W4, d.E8 = L.ptr(W4), L.ptr(E8)
    if norm_w is not None:
        d.norm_w, d.eps = L.ptr(norm_w), eps
    N = Wr.shape[0] // 2 if mode == 1 else Wr.shape[0]
    d.N = N
    if out is None:
        out = torch.empty(M, dq if mode == 2 and not raw_qkv else N, device=A.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    d.C, d.ldc, d.out_f32 = L.ptr(out), _ld(out), int(out.dtype == torch.float32)
    if R is not None:
        d.R, d.ldr = L.ptr(R), _ld(R)
    if mode == 2 and raw_qkv:
        d.dq, d.dkv, d.hd, d.raw_qkv = dq, dkv, hd, 1
    elif mode == 2:
        d.dq, d.dkv, d.hd, d.rope, d.kc, d.vc, d.Tmax, d.pos = dq, dkv, hd, L.ptr(rope), L.ptr(kc), L.ptr(vc), kc.shape[1], pos
        d.pos_dev = L.ptr(pos_dev)
    if lora_t is not None:          # adapters: lora_t [M, >= 64 per module] f32 rank-side products, lora_b = padded B images [rows, 64] (one, or q / k / v)
        d.lora_t, d.ld_lora_t, d.lora_r, d.lora_scale = L.ptr(lora_t), _ld(lora_t), lora_r, lora_scale
        for j, b in enumerate(lora_b):
            d.lora_b[j] = L.ptr(b)
    if bias is not None:
        if bias.dtype != torch.bfloat16 or bias.numel() != N or not bias.is_contiguous():
            raise ValueError(f"dec_proj: bias must be a contiguous bf16 [{N}] tensor")
        d.bias = L.ptr(bias)
    L.check(L.load().avllm_dec_proj(C.byref(d), L.stream_ptr()))
    return out


def attention_decode(q, kc, vc, H, Tk, tk_dev=None, scale=None):
    """q [B, H*hd]; kc, vc [B, Tmax, Hkv*hd] -> [B, H*hd]: softmax(q.K^T * scale) V over cache rows [0, Tk (+ *tk_dev))."""
    B, d = q.shape
    hd = d // H
    Hkv = kc.shape[2] // hd
    o = torch.empty_like(q)
    L.check(L.load().avllm_attention_decode(L.ptr(q), _ld(q), L.ptr(kc), L.ptr(vc), L.ptr(o), _ld(o), B, H, hd, Tk, L.ptr(tk_dev), kc.shape[1],
                                            float(scale if scale is not None else hd ** -0.5), H // Hkv, L.dt_of(q), L.stream_ptr()))
    return o


# ---------------------------------------------------------------- fp8 KV cache (csrc/kv_fp8.hip)
# A cache image is ONE uint8 tensor of shape [..., dkv + dkv/32] whose BYTES are two planes: the codes of all rows, [..., dkv], then the
# exponents of all rows, [..., dkv/32].  The shape only carries the sizes (rows, Tmax, dkv); read an image through kv8_unpack.
def kv8_alloc(*lead, dkv, device="cuda"):
    """An uninitialised image of cache rows [*lead, dkv]."""
    if dkv % 32:
        raise ValueError(f"kv8: dkv = {dkv} must be a multiple of 32")
    return torch.empty(*lead, dkv + dkv // 32, dtype=torch.uint8, device=device)


def kv8_dkv(cache):
    if cache.dtype != torch.uint8 or not cache.is_contiguous() or cache.shape[-1] % 33:
        raise ValueError("kv8: a cache image is a contiguous uint8 tensor [..., dkv + dkv/32]")
    return cache.shape[-1] // 33 * 32


def kv8_unpack(cache):
    """-> (codes uint8 [..., dkv], exponents uint8 [..., dkv/32]): views of the image's two planes."""
    dkv = kv8_dkv(cache)
    n = cache.numel() // 33 * 32
    flat = cache.view(-1)
    return flat[:n].view(*cache.shape[:-1], dkv), flat[n:].view(*cache.shape[:-1], dkv // 32)


def kv8_pack(codes, exponents):
    """The image of codes uint8 [..., dkv] and exponents uint8 [..., dkv/32] (a new tensor)."""
    dkv = codes.shape[-1]
    if codes.dtype != torch.uint8 or exponents.dtype != torch.uint8 or exponents.shape != codes.shape[:-1] + (dkv // 32,) or dkv % 32:
        raise ValueError("kv8_pack: codes uint8 [..., dkv] and exponents uint8 [..., dkv/32]")
    cache = kv8_alloc(*codes.shape[:-1], dkv=dkv, device=codes.device)
    q, e = kv8_unpack(cache)
    q.copy_(codes)
    e.copy_(exponents)
    return cache


def _kv8_planes(cache):
    q, e = kv8_unpack(cache)
    return L.ptr(q), L.ptr(e)


def kv8_append(k, v, kc, vc, T, pos0):
    """kv_append onto the fp8 images kc, vc of cache rows [B, Tmax, dkv]: rows k, v [B*T, dkv] (bf16 views with one row stride) are stored by
    the MX rule at positions [pos0, pos0 + T) (avllm_kv8_append)."""
    B, Tmax, dkv = kc.shape[0], kc.shape[1], kv8_dkv(kc)
    assert kc.dim() == 3 and vc.shape == kc.shape and k.shape == (B * T, dkv) and v.shape == k.shape and _ld(k) == _ld(v) and k.dtype == torch.bfloat16
    L.check(L.load().avllm_kv8_append(L.ptr(k), L.ptr(v), _ld(k), *_kv8_planes(kc), *_kv8_planes(vc), B, T, pos0, Tmax, dkv, L.stream_ptr()))


def kv8_rope_append_(qkv, heads, kv_heads, hd, rope, kc, vc, pos=0, pos_dev=None, rotate=True):
    """The token step's append (avllm_kv8_rope_append) on the raw q|k|v rows qkv [B, ld] (bf16): q rotated in place, k rotated and quantised,
    v quantised, the row written at pos (+ *pos_dev) of the images kc, vc of [B, Tmax, kv_heads hd].  rotate=False: q and k are rotated already."""
    B, Tmax = kc.shape[0], kc.shape[1]
    assert kc.dim() == 3 and vc.shape == kc.shape and kv8_dkv(kc) == kv_heads * hd and qkv.shape[0] == B and qkv.dtype == torch.bfloat16
    assert rope is None or (rope.dtype == torch.float32 and rope.is_contiguous() and rope.numel() == hd)
    L.check(L.load().avllm_kv8_rope_append(L.ptr(qkv), _ld(qkv), B, heads, kv_heads, hd, L.ptr(rope), int(rotate), *_kv8_planes(kc), *_kv8_planes(vc),
                                           Tmax, pos, L.ptr(pos_dev), L.stream_ptr()))
    return qkv


def attention_decode_kv8(q, kc, vc, H, Tk, tk_dev=None, scale=None):
    """attention_decode over the fp8 images kc, vc of [B, Tmax, Hkv*hd]; q [B, H*hd] bf16 -> [B, H*hd] (avllm_attention_decode_kv8)."""
    B, d = q.shape
    hd = d // H
    Hkv = kv8_dkv(kc) // hd
    assert kc.dim() == 3 and vc.shape == kc.shape and kc.shape[0] == B and q.dtype == torch.bfloat16
    o = torch.empty_like(q)
    L.check(L.load().avllm_attention_decode_kv8(L.ptr(q), _ld(q), *_kv8_planes(kc), *_kv8_planes(vc), L.ptr(o), _ld(o), B, H, hd, Tk, L.ptr(tk_dev),
                                                kc.shape[1], float(scale if scale is not None else hd ** -0.5), H // Hkv, L.stream_ptr()))
    return o


def _shared_args(name, q, k_prefix, v_prefix, S, k_suffix, v_suffix, H, n, group, tk_dev):
    """The checks both cache forms of attention_decode_shared share -> (R, hd, N, workspace)."""
    if q.dim() != 2 or q.dtype != torch.bfloat16:
        raise ValueError(f"{name}: q must be bf16 [R, H*hd], got {tuple(q.shape)} {q.dtype}")
    R, hd = q.shape[0], q.shape[1] // H
    for what, t, rows in (("k_prefix", k_prefix, None), ("v_prefix", v_prefix, None), ("k_suffix", k_suffix, R), ("v_suffix", v_suffix, R)):
        if t.dim() != 3 or not t.is_contiguous() or (rows is not None and t.shape[0] != rows):
            raise ValueError(f"{name}: {what} must be a contiguous cache [{'R' if rows else 'B'}, T, dkv], got {tuple(t.shape)}")
    if k_prefix.shape != v_prefix.shape or k_suffix.shape != v_suffix.shape or k_prefix.dtype != k_suffix.dtype:
        raise ValueError(f"{name}: the K and V caches of the prefix, and of the suffix, must have one shape each and all one dtype")
    if group < 1 or R != k_prefix.shape[0] * group:
        raise ValueError(f"{name}: group = {group} rows per item of the {k_prefix.shape[0]}-row prefix cache, but q has {R} rows")
    N = k_suffix.shape[1]
    if tk_dev is None and not 0 <= n < N:
        raise ValueError(f"{name}: n = {n} outside the suffix cache (N = {N})")
    ws = torch.empty(L.load().avllm_attention_decode_shared_workspace_bytes(R, H, hd), dtype=torch.uint8, device=q.device)
    return R, hd, N, ws


def attention_decode_shared(q, k_prefix, v_prefix, S, k_suffix, v_suffix, H, n, group, tk_dev=None, scale=None):
    """q [R, H*hd] bf16, R = B*group; k_prefix, v_prefix [B, Tp, Hkv*hd]; k_suffix, v_suffix [R, N, Hkv*hd] -> [R, H*hd]: row r attends rows
    [0, S) of item r // group of the prefix cache, then rows [0, n] (+ *tk_dev, clamped to N) of its own suffix rows
    (avllm_attention_decode_shared)."""
    R, hd, N, ws = _shared_args("attention_decode_shared", q, k_prefix, v_prefix, S, k_suffix, v_suffix, H, n, group, tk_dev)
    if k_prefix.dtype != torch.bfloat16:
        raise ValueError(f"attention_decode_shared: caches must be bf16 (fp8 images: attention_decode_shared_kv8), got {k_prefix.dtype}")
    Hkv = k_prefix.shape[2] // hd
    o = torch.empty_like(q)
    L.check(L.load().avllm_attention_decode_shared(L.ptr(q), _ld(q), L.ptr(k_prefix), L.ptr(v_prefix), S, k_prefix.shape[1], L.ptr(k_suffix), L.ptr(v_suffix),
                                                   n + 1, L.ptr(tk_dev), N, L.ptr(o), _ld(o), R, group, H, hd,
                                                   float(scale if scale is not None else hd ** -0.5), H // Hkv, L.ptr(ws), ws.numel(), L.stream_ptr()))
    return o


def attention_decode_shared_kv8(q, k_prefix, v_prefix, S, k_suffix, v_suffix, H, n, group, tk_dev=None, scale=None):
    """attention_decode_shared over fp8 images: k_prefix, v_prefix of [B, Tp, Hkv*hd], k_suffix, v_suffix of [R, N, Hkv*hd]
    (avllm_attention_decode_shared_kv8)."""
    R, hd, N, ws = _shared_args("attention_decode_shared_kv8", q, k_prefix, v_prefix, S, k_suffix, v_suffix, H, n, group, tk_dev)
    Hkv = kv8_dkv(k_prefix) // hd
    if kv8_dkv(k_suffix) != Hkv * hd:
        raise ValueError("attention_decode_shared_kv8: prefix and suffix images differ in dkv")
    o = torch.empty_like(q)
    L.check(L.load().avllm_attention_decode_shared_kv8(L.ptr(q), _ld(q), *_kv8_planes(k_prefix), *_kv8_planes(v_prefix), S, k_prefix.shape[1],
                                                       *_kv8_planes(k_suffix), *_kv8_planes(v_suffix), n + 1, L.ptr(tk_dev), N, L.ptr(o), _ld(o), R, group, H,
                                                       hd, float(scale if scale is not None else hd ** -0.5), H // Hkv, L.ptr(ws), ws.numel(),
                                                       L.stream_ptr()))
    return o


def kv8_gather_rows(k_src, v_src, k_dst, v_dst, parent, t0, t1):
    """kv_gather_rows on fp8 images of [layers, rows, T, dkv]: codes and exponents of positions [t0, t1) move together
    (avllm_kv8_gather_rows)."""
    for t in (k_src, v_src, k_dst, v_dst):
        if not (t.is_cuda and t.dim() == 4):
            raise ValueError("kv8_gather_rows: caches must be 4-d device images [layers, rows, T, dkv + dkv/32]")
        kv8_dkv(t)
    if k_src.shape != v_src.shape or k_dst.shape != v_dst.shape:
        raise ValueError("kv8_gather_rows: K and V caches must have equal shapes")
    (Ls, Rs, Ts, _), (Ld, Rd, Td, _) = k_src.shape, k_dst.shape
    D = kv8_dkv(k_src)
    if Ls != Ld or D != kv8_dkv(k_dst):
        raise ValueError(f"kv8_gather_rows: src {tuple(k_src.shape)} and dst {tuple(k_dst.shape)} differ in layers or width")
    if (k_src.data_ptr() == k_dst.data_ptr()) != (v_src.data_ptr() == v_dst.data_ptr()):
        raise ValueError("kv8_gather_rows: K and V must both be in place or both out of place")
    if not (parent.is_cuda and parent.dtype == torch.int32 and parent.is_contiguous() and parent.shape == (Rd,)):
        raise ValueError(f"kv8_gather_rows: parent must be a contiguous int32 device tensor [{Rd}]")
    if not 0 <= t0 <= t1 <= min(Ts, Td):
        raise ValueError(f"kv8_gather_rows: positions [{t0}, {t1}) outside the caches (T = {Ts}, {Td})")
    L.check(L.load().avllm_kv8_gather_rows(L.ptr(k_src), L.ptr(v_src), Rs, Ts, L.ptr(k_dst), L.ptr(v_dst), Rd, Td, Ls, D, L.ptr(parent), t0, t1,
                                           L.stream_ptr()))


def step_advance(state, base_lr, total_steps, warmup_steps=0, beta1=0.9, beta2=0.95, rank=0):
    """One-thread kernel: state.step += 1 and this step's lr / bias corrections / dropout seed (include/avllm.h avllm_step_state)."""
    sc = L.Schedule(base_lr, beta1, beta2, int(warmup_steps), int(total_steps), int(rank))
    L.check(L.load().avllm_step_advance(L.ptr(state), C.byref(sc), L.stream_ptr()))


MICRO_SEED_STRIDE = 0xC2B2AE35          # AVLLM_MICRO_SEED_STRIDE of include/avllm.h


def step_advance_micro(state, base_lr, total_steps, warmup_steps=0, beta1=0.9, beta2=0.95, rank=0):
    """The micro-step form (avllm_step_advance_micro): advances the optimizer step only when the window's micro-step count (state.reserved[0])
    is 0, gives every micro-step its own dropout seed, then counts the micro-step."""
    sc = L.Schedule(base_lr, beta1, beta2, int(warmup_steps), int(total_steps), int(rank))
    L.check(L.load().avllm_step_advance_micro(L.ptr(state), C.byref(sc), L.stream_ptr()))


def window_add(window, acc, state):
    """window [loss_sum, count] += acc, in a fixed order on the device; overwritten at the first micro-step of a window (avllm_window_add)."""
    if window.dtype != torch.float32 or acc.dtype != torch.float32 or window.numel() != 2 or acc.numel() != 2:
        raise ValueError("window_add: window and acc must be float32 tensors of two elements")
    L.check(L.load().avllm_window_add(L.ptr(window), L.ptr(acc), L.ptr(state), L.stream_ptr()))


def whisper_im2col1(mel, Kpad, dtype):
    B, n_mels, T = mel.shape
    cols = torch.empty(B * T, Kpad, device=mel.device, dtype=dtype)
    L.check(L.load().avllm_whisper_im2col1(L.ptr(mel), L.ptr(cols), B, n_mels, T, Kpad, L.dt_of(cols), L.stream_ptr()))
    return cols


def whisper_im2col2(h, B, T):
    d = h.shape[-1]
    cols = torch.empty(B * (T // 2), 3 * d, device=h.device, dtype=h.dtype)
    L.check(L.load().avllm_whisper_im2col2(L.ptr(h), L.ptr(cols), B, T, d, L.dt_of(h), L.stream_ptr()))
    return cols


def clip_patchify(frames, patch, Kpad, dtype):
    N, _, S, _ = frames.shape
    g = S // patch
    cols = torch.empty(N * g * g, Kpad, device=frames.device, dtype=dtype)
    L.check(L.load().avllm_clip_patchify(L.ptr(frames), L.ptr(cols), N, S, patch, Kpad, L.dt_of(cols), L.stream_ptr()))
    return cols


def dropout(x, seed, p):
    """y = x * keep/(1-p) with the library's counter-based mask (avllm_dropout)."""
    x = x.contiguous()
    y = torch.empty_like(x)
    L.check(L.load().avllm_dropout(L.ptr(x), L.ptr(y), x.numel() // x.shape[-1], x.shape[-1], seed & 0xFFFFFFFF, p, L.dt_of(x), L.stream_ptr()))
    return y
