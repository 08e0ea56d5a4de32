"""Restatements of the connector-training kernels (avllm_fuse_pool_bwd, avllm_gemm_wgrad) in plain torch, float64 by default (dtype=float32
gives the same arithmetic on the host in fp32: the measurement tests/bars.py's fp32_bar starts from).  tests/test_connector_refs_cpu.py pins
them to autograd through the oracle's pad_or_truncate / adaptive_projection and to dY.T @ X."""
import torch


def pool_matrix(Lt, S_out, dtype=torch.float64):
    """W [S_out, Lt] with out = W @ X for the three branches of avllm_fuse_pool (clip_whisper_model.py:621-707): identity, AdaptiveAvgPool1d
    windows [floor(i Lt / S), ceil((i + 1) Lt / S)), linear interpolation with align_corners=True (source position i (Lt - 1) / (S - 1))."""
    W = torch.zeros(S_out, Lt, dtype=dtype)
    if Lt == S_out:
        W += torch.eye(Lt, dtype=dtype)
    elif Lt > S_out:
        for i in range(S_out):
            s, e = (i * Lt) // S_out, -((-(i + 1) * Lt) // S_out)
            W[i, s:e] = torch.ones((), dtype=dtype) / (e - s)
    else:
        scale = torch.tensor(Lt - 1, dtype=dtype) / (S_out - 1) if S_out > 1 else torch.zeros((), dtype=dtype)
        for i in range(S_out):
            src = scale * i
            lo = int(src)
            hi = min(lo + 1, Lt - 1)
            w1 = src - lo
            W[i, lo] += 1 - w1
            W[i, hi] += w1
    return W


def fuse_pool_bwd(dx, Ta, Tv, P, L, fs, dtype=torch.float64):
    """dx [B,S_out,D] -> (da [B,Ta,D] | None, dv [B,Tv,D] | None): the adjoint of the virtual sequence [prompt ; fs a + (1 - fs) v] pooled to S_out
    rows.  Rows t >= L of an input are zero; the prompt's P rows are dropped; one input alone carries scale 1."""
    dx = dx.to(dtype)
    B, S_out, D = dx.shape
    W = pool_matrix(P + L, S_out, dtype)
    g = torch.einsum("ij,bid->bjd", W, dx)[:, P:]                     # [B, L, D]: gradient of the fused rows
    both = Ta > 0 and Tv > 0

    def side(T, w):
        if not T:
            return None
        out = torch.zeros(B, T, D, dtype=dtype)
        n = min(T, L)
        out[:, :n] = (w * g[:, :n]) if both else g[:, :n]
        return out
    return side(Ta, torch.tensor(fs, dtype=torch.float32).to(dtype)), side(Tv, (1 - torch.tensor(fs, dtype=torch.float32)).to(dtype))


def gemm_wgrad(dY, X, alpha=1.0, dtype=torch.float64):
    """(dW [N,K], db [N]) = alpha * (dY^T X, column sums of dY)."""
    dY, X = dY.to(dtype), X.to(dtype)
    return alpha * (dY.t() @ X), alpha * dY.sum(0)
