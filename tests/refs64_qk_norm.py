"""Float64 restatements of avllm_qk_norm_rope and avllm_qk_norm_bwd (csrc/qk_norm.hip), the families their tests run and the operands
of the locate family.  tests/test_qwen3_cpu.py pins both to torch.autograd in float64 and shows that the restatement run in float32 stays
inside the bars of tests/bars_qk_norm.py; tests/test_qk_norm_pin_gpu.py holds the kernels to them.  The per-head norm is transformers'
Qwen3RMSNorm on q_proj(x).view(.., hd): y = x * rsqrt(mean(x^2) + eps) * w, then apply_rotary_pos_emb: pairs (i, i + hd/2)."""
import zlib
from types import SimpleNamespace

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS = 1e-6
GEOMETRY = ((14, 2, 64), (4, 2, 128), (2, 2, 128))          # (H, Hkv, hd)
FAMILIES = ("gauss", "offset", "tiny", "locate")
PAD = 24                                                    # columns past q|k|v: ld is larger than the used width


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def stored(t, dtype):
    """The values a tensor of the storage dtype holds, as float32."""
    return t.to(dtype).to(F32)


def table(T, hd, pos0, theta=1e6):
    """[T, hd/2, 2] fp32 (cos, sin) of the fp32 angle (pos0 + t) * inv_freq_i: the table both sides read."""
    inv = 1.0 / (torch.tensor(theta, dtype=F32) ** (torch.arange(0, hd, 2, dtype=torch.int64).to(F32) / hd))
    ang = ((pos0 + torch.arange(T, dtype=F32))[:, None] * inv[None, :]).to(F64)
    return torch.stack([ang.cos(), ang.sin()], -1).to(F32).contiguous()


def weights(fam, hd, dtype):
    """(q's, k's) norm vectors.  locate: distinct per index and disjoint between q and k, every value a bf16 value: wq[i] = 1 + i / 64 in
    [1, 3), wk[i] = 4 + i / 32 in [4, 8)."""
    i = torch.arange(hd, dtype=F32)
    if fam == "locate":
        return stored(1.0 + i / 64.0, dtype), stored(4.0 + i / 32.0, dtype)
    g = gen("w", fam, hd)
    return stored(1.0 + 0.3 * torch.randn(hd, generator=g), dtype), stored(1.0 + 0.3 * torch.randn(hd, generator=g), dtype)


def inputs(fam, M, H, Hkv, hd, dtype, what="x"):
    """[M, (H + 2 Hkv) hd + PAD] in the storage dtype's values: the q|k|v buffer (or its gradient) with padding columns."""
    ld = (H + 2 * Hkv) * hd + PAD
    g = gen(what, fam, M, H, Hkv, hd)
    if fam == "gauss":
        x = torch.randn(M, ld, generator=g)
    elif fam == "offset":                                   # |mean| >> sigma inside a head
        x = 8.0 + 0.05 * torch.randn(M, ld, generator=g)
    elif fam == "tiny":                                     # mean(x^2) of the size of eps
        x = 1e-3 * torch.randn(M, ld, generator=g)
    else:                                                   # locate: small integers
        x = torch.randint(-4, 5, (M, ld), generator=g).float()
    return stored(x, dtype)


def _heads(x, M, NQK, hd, dtype):
    return x[:, :NQK * hd].to(dtype).reshape(M, NQK, hd)


def _w(wq, wk, H, Hkv, dtype):
    return torch.cat([wq.to(dtype)[None].expand(H, -1), wk.to(dtype)[None].expand(Hkv, -1)], 0)


def fwd64(x, H, Hkv, hd, wq, wk, eps, tab, dtype=F64):
    """-> namespace: out [M, (H + Hkv) hd] (normed and rotated q|k), rstd [M, H + Hkv], and for the bars y (normed, before the rotation)
    [M, NQK, hd] with the table's cos / sin broadcast against its halves."""
    M, NQK, half = x.shape[0], H + Hkv, hd // 2
    X = _heads(x, M, NQK, hd, dtype)
    rstd = torch.rsqrt((X * X).mean(-1) + eps)
    y = X * rstd[..., None] * _w(wq, wk, H, Hkv, dtype)[None]
    t = torch.arange(M) % tab.shape[0]
    c, s = tab[t, :, 0].to(dtype)[:, None, :], tab[t, :, 1].to(dtype)[:, None, :]
    a, b = y[..., :half], y[..., half:]
    out = torch.cat([a * c - b * s, b * c + a * s], -1)
    return SimpleNamespace(out=out.reshape(M, NQK * hd), rstd=rstd, y=y, c=c, s=s, hd=hd)


def bwd64(dy, pre, rstd, H, Hkv, hd, wq, wk, dtype=F64):
    """dx [M, (H + Hkv) hd] from dy (the gradient of the normed pre-RoPE heads; a [M, >= NQK hd] buffer), the saved pre-norm values
    [M, NQK hd] and the saved rstd [M, NQK], which is an INPUT here as it is for the kernel.  -> namespace: dx, g, xh."""
    M, NQK = dy.shape[0], H + Hkv
    D, X, r = _heads(dy, M, NQK, hd, dtype), _heads(pre, M, NQK, hd, dtype), rstd.to(dtype)[..., None]
    g, xh = _w(wq, wk, H, Hkv, dtype)[None] * D, X * r
    dx = r * (g - xh * (g * xh).mean(-1, keepdim=True))
    return SimpleNamespace(dx=dx.reshape(M, NQK * hd), g=g, xh=xh, rstd=rstd.to(dtype))


def radial(pre, rstd, H, Hkv, hd):
    """The family whose exact result is (up to eps) 0: w = 1 and dy = pre, so g = x is parallel to xhat = x rstd exactly, in every storage
    dtype.  -> (dy buffer values = pre's, unit weights)."""
    return pre.clone(), torch.ones(hd), torch.ones(hd)
