"""Restatements of the per-clip modality kernels (csrc/modality.hip): avllm_fuse_pool_rows and its adjoint in plain torch through
refs64_connector.pool_matrix, float64 by default (dtype=float32: the same arithmetic on the host in fp32, which tests/bars.py's fp32_bar starts
from), and the draw rule of avllm_modality_draw in pure Python integers.  tests/test_modality_refs_cpu.py pins the adjoint to autograd through
the forward and the draw to its edge cases and frequencies."""
import struct

import torch

from refs64_connector import pool_matrix

BOTH, AUDIO, VIDEO = 0, 1, 2
M32 = 0xFFFFFFFF
DRAW_OFFSET = 0x6D6F6461


def _scales(fs, dtype):
    f = torch.tensor(fs, dtype=torch.float32)
    return f.to(dtype), (1 - f).to(dtype)


def fused_rows(a, v, modes, L, fs, dtype=torch.float64):
    """[B, L, D]: row t of clip b is fs a + (1 - fs) v (mode 0), a (mode 1) or v (mode 2), each input zero past its length.  The stream a clip
    does not use is not touched (it may hold NaN)."""
    B, Ta, D = a.shape
    Tv = v.shape[1]
    wa, wv = _scales(fs, dtype)
    out = torch.zeros(B, L, D, dtype=dtype)
    na, nv = min(Ta, L), min(Tv, L)
    for b, m in enumerate(modes):
        m = m if m in (AUDIO, VIDEO) else BOTH
        if m == BOTH:
            out[b, :na] = wa * a[b, :na].to(dtype)
            out[b, :nv] = out[b, :nv] + wv * v[b, :nv].to(dtype)
        elif m == AUDIO:
            out[b, :na] = a[b, :na].to(dtype)
        else:
            out[b, :nv] = v[b, :nv].to(dtype)
    return out


def fuse_pool_rows(a, v, pe, modes, L, S_out, fs, dtype=torch.float64):
    """a [B,Ta,D], v [B,Tv,D], pe [B,P,D] | None, modes a list of B ints -> out [B,S_out,D]."""
    x = fused_rows(a, v, modes, L, fs, dtype)
    if pe is not None:
        x = torch.cat([pe.to(dtype), x], dim=1)
    W = pool_matrix(x.shape[1], S_out, dtype)
    return torch.einsum("ij,bjd->bid", W, x)


def fuse_pool_rows_bwd(dx, modes, Ta, Tv, P, L, fs, dtype=torch.float64):
    """dx [B,S_out,D] -> (da [B,Ta,D], dv [B,Tv,D]): a clip's used stream carries scale 1 (modes 1, 2) or fs / 1 - fs (mode 0), its unused
    stream zeros; rows t >= L are zeros; the prompt's P rows are dropped."""
    dx = dx.to(dtype)
    B, S_out, D = dx.shape
    W = pool_matrix(P + L, S_out, dtype)
    g = torch.einsum("ij,bid->bjd", W, dx)[:, P:]
    wa, wv = _scales(fs, dtype)
    da, dv = torch.zeros(B, Ta, D, dtype=dtype), torch.zeros(B, Tv, D, dtype=dtype)
    na, nv = min(Ta, L), min(Tv, L)
    for b, m in enumerate(modes):
        m = m if m in (AUDIO, VIDEO) else BOTH
        if m == BOTH:
            da[b, :na], dv[b, :nv] = wa * g[b, :na], wv * g[b, :nv]
        elif m == AUDIO:
            da[b, :na] = g[b, :na]
        else:
            dv[b, :nv] = g[b, :nv]
    return da, dv


# ---------------------------------------------------------------- the draw (include/avllm.h, avllm_modality_draw)
def av_hash32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def av_pair_hash(seed, pair):
    hi = (pair >> 32) & M32
    inner = av_hash32((seed + hi * 0x9E3779B9) & M32)         # hi == 0: av_hash32(seed)
    return av_hash32((pair & M32) ^ inner)


def threshold(p):
    """(uint32_t)(p * 2^24 + 0.5) of the FLOAT argument p, evaluated in double."""
    p32 = struct.unpack("f", struct.pack("f", float(p)))[0]
    return int(p32 * 16777216.0 + 0.5)


def draw(B, p_drop_audio, p_drop_video, seed, mode_in=None):
    """The modes of B clips for the launch seed `seed` (seed_dev word + by-value seed, mod 2^32)."""
    ta, tv = threshold(p_drop_audio), threshold(p_drop_video)
    s = (seed + DRAW_OFFSET) & M32
    out = []
    for b in range(B):
        if mode_in is not None and mode_in[b] in (AUDIO, VIDEO):
            out.append(int(mode_in[b]))
            continue
        u = av_pair_hash(s, b) >> 8
        out.append(VIDEO if u < ta else (AUDIO if u >= (1 << 24) - tv else BOTH))
    return out


def step_seed(step, rank=0, skipped=0):
    """avllm_step_state.dropout_seed of optimizer step `step` (1-based), also the host seed of the model's step-th training forward."""
    return ((step + skipped) * 0x9E3779B1 + rank * 0x85EBCA6B + 12345) & M32
