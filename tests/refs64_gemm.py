"""Plain float64 restatements of the GEMM family (csrc/gemm.hip, gemm_dp.hip, gemm_tn.hip, gemm_tn_kernel of loss_optim.hip), the dropout mask of
csrc/common.h restated in numpy integer arithmetic, the deterministic input families, a host emulation of the documented arithmetic with the
mutants tests/test_gemm_refs_cpu.py builds from it, and the geometry / epilogue tables of tests/test_gemm_pin_gpu.py.

gemm() is the whole formula of avllm_gemm as gemm.hip's header states it: act(alpha (A B^T + A2 B2^T) + bias), then the dropout mask, then + R,
then the row remap.  Operands are taken as the kernel sees them (bf16 tensors are upcast, never re-drawn).  Nothing here touches the GPU."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_SILU = 0, 1, 2, 3
LOG2E = 1.4426950408889634


def _c(t, dtype):
    return None if t is None else t.detach().to("cpu").to(dtype)


# ------------------------------------------------------------------------------------------------ the dropout mask (common.h), in numpy integers
_M32 = np.uint64(0xFFFFFFFF)


def _hash32(x):
    """av_hash32 (lowbias32) on uint64 arrays holding 32-bit values."""
    x = x & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def drop_thr(p):
    """av_drop_thr: (uint32)(p * 65536.0f), the product formed in fp32."""
    return int(np.float32(p) * np.float32(65536.0))


def drop_scale(p):
    """av_drop_scale: 1.0f / (1.0f - (float)thr * (1.0f / 65536.0f)), every operation in fp32; returned as a Python float holding that fp32 value."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(drop_thr(p)) * np.float32(1.0 / 65536.0)))


def pair_hash(seed, pair):
    """av_pair_hash: pair a uint64 array.  The inner avalanche is av_hash32(seed) while the pair index fits 32 bits, av_hash32(seed + hi * 0x9E3779B9)
    beyond (the high-word branch)."""
    pair = np.asarray(pair, dtype=np.uint64)
    hi = pair >> np.uint64(32)
    seed = np.uint64(seed & 0xFFFFFFFF)
    inner = np.where(hi != 0, _hash32((seed + ((hi * np.uint64(0x9E3779B9)) & _M32)) & _M32), _hash32(np.asarray(seed)))
    return _hash32((pair & _M32) ^ inner)


def keep(seed, idx, p):
    """av_keep(seed, idx, p) -> bool array of idx's shape.  idx: anything numpy turns into uint64."""
    idx = np.asarray(idx, dtype=np.uint64)
    h = pair_hash(seed, idx >> np.uint64(1))
    half = np.where((idx & np.uint64(1)) != 0, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return half >= np.uint64(drop_thr(p))


@functools.lru_cache(maxsize=16)
def keep_grid(seed, rows, cols, stride, p):
    """(cached: callers do not write to the result)  keep over the index row * stride + col for row < rows, col < cols -> torch bool [rows, cols]."""
    idx = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(stride) + np.arange(cols, dtype=np.uint64)[None, :]
    return torch.from_numpy(keep(seed, idx, p))


def dropped_operand(X, seed, p, stride=None):
    """dropout(X) as the fused A-operand mask and gemm_tn_drop form it: keep on index row * stride + col, survivors times the fp32 scale in fp32,
    re-rounded to bf16.  -> float64."""
    X = _c(X, F64)
    rows, cols = X.shape
    k = keep_grid(seed, rows, cols, cols if stride is None else stride, p)
    scaled = (X * drop_scale(p)).to(F32).to(BF16).to(F64)          # bf16 x fp32 is exact in float64: one rounding to fp32, one to bf16, as on the device
    return torch.where(k, scaled, torch.zeros_like(scaled))


# ------------------------------------------------------------------------------------------------ activations
def act64(z, act):
    if act == ACT_GELU:
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if act == ACT_QUICK_GELU:
        return z * torch.sigmoid(1.702 * z)
    if act == ACT_SILU:
        return z * torch.sigmoid(z)
    return z


def dact64(z, act):
    if act == ACT_GELU:
        return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    if act in (ACT_QUICK_GELU, ACT_SILU):
        k = 1.702 if act == ACT_QUICK_GELU else 1.0
        s = torch.sigmoid(k * z)
        return s + k * z * s * (1 - s)
    return torch.ones_like(z)


# ------------------------------------------------------------------------------------------------ the references
Ref = namedtuple("Ref", "out sum_abs z acc rows mask")      # out [M, N] by LOGICAL row, rows [M] = the output row of each, mask = keep * scale or None


def out_rows(M, remap):
    m = torch.arange(M)
    if remap is None:
        return m
    g_in, g_out, g_off = remap
    return (m // g_in) * g_out + g_off + m % g_in


def gemm(A, B, A2=None, B2=None, bias=None, R=None, act=ACT_NONE, alpha=1.0, r_mod=0, remap=None, drop=None, a_drop=None, n_valid=0, dtype=F64):
    A_, B_ = _c(A, dtype), _c(B, dtype)
    M, K = A_.shape
    N = B_.shape[0]
    if a_drop is not None:
        A_ = dropped_operand(A, a_drop[0], a_drop[1]).to(dtype)
    acc = A_ @ B_.t()
    sa = A_.abs() @ B_.abs().t()
    if A2 is not None:
        acc = acc + _c(A2, dtype) @ _c(B2, dtype).t()
        sa = sa + _c(A2, dtype).abs() @ _c(B2, dtype).abs().t()
    if n_valid > 0:                                    # the rank-side kernel streams only the 16-column groups that hold values; the rest is written 0
        nv = 16 * ((n_valid + 15) // 16)
        acc[:, nv:] = 0
        sa[:, nv:] = 0
    z = alpha * acc
    if bias is not None:
        z = z + _c(bias, dtype)[None, :]
    y = act64(z, act)
    mask = None
    if drop is not None:
        mask = keep_grid(drop[0], M, N, N, drop[1]).to(dtype) * drop_scale(drop[1])
        y = y * mask
    if R is not None:
        rr = torch.arange(M) % r_mod if r_mod > 0 else torch.arange(M)
        y = y + _c(R, dtype)[rr]
    return Ref(y, sa, z, acc, out_rows(M, remap), mask)


RefTN = namedtuple("RefTN", "out sum_abs acc")


def tn_big_is_p(I, J):
    """Which operand av_gemm_tn treats as the wide one (the one a drop masks): P when J <= 16 and I % 128 == 0, else Q."""
    return J <= 16 and I % 128 == 0


def gemm_tn(P, Q, I=None, J=None, alpha=1.0, drop=None, out=None, dtype=F64):
    """out[I, J] + alpha * P[:, :I]^T Q[:, :J]; drop = (seed, p) masks the wide operand on index row * width + col."""
    I = P.shape[1] if I is None else I
    J = Q.shape[1] if J is None else J
    P_, Q_ = _c(P, dtype)[:, :I], _c(Q, dtype)[:, :J]
    if drop is not None:
        if tn_big_is_p(I, J):
            P_ = dropped_operand(P_, drop[0], drop[1]).to(dtype)
        else:
            Q_ = dropped_operand(Q_, drop[0], drop[1]).to(dtype)
    acc = P_.t() @ Q_
    sa = P_.abs().t() @ Q_.abs()
    o = alpha * acc
    if out is not None:
        o = o + _c(out, dtype)
    return RefTN(o, sa, acc)


# ------------------------------------------------------------------------------------------------ input families (every value bf16-exact, fp32 tensors)
FAMILIES = ("randn", "offset", "heavy", "exact", "locate")
ZERO_BAR = ("exact", "locate")
EXACT_NNZ = 64          # non-zeros (+-1) per row of [A | A2]; B in {+-1, +-2}: |acc| <= 128, so alpha acc + bias + R (|bias|, |R| <= 8) is an integer <= 144 or a
                        # half-integer <= 80: both exact in bf16 (8 significant bits) at every K, which exact_holds() checks on the reference alone


def _bf(x):
    return x.to(BF16).to(F32)


def _gen(*key):
    g = torch.Generator()
    g.manual_seed(abs(hash(tuple(int(k) if not isinstance(k, str) else sum(map(ord, k)) for k in key))) % (2 ** 31))
    return g


def locate_column(M, KK):
    """f(m): the hot column of row m.  With M >= K + K2 it sweeps every k; with fewer rows it strides through both segments."""
    step = max(1, KK // max(M, 1)) | 1 if M < KK else 1
    return (torch.arange(M) * step) % KK


def locate_code(N, KK):
    """B's integer code of (n, k): asymmetric in (n, k), |code| <= 100, so that 2 code + R (the p = 0.5 mask, |R| <= 8) stays a bf16 integer."""
    n, k = torch.arange(N)[:, None], torch.arange(KK)[None, :]
    return (((3 * n + 7 * k) % 201) - 100).to(F32)


def family(fam, M, N, K, K2=0, r_rows=None, seed=0):
    """-> dict A [M,K], B [N,K], A2 / B2 [., K2] or None, bias [N], R [r_rows or M, N]: fp32 tensors of bf16-exact values."""
    g = _gen(fam, M, N, K, K2, seed)
    KK = K + K2
    rr = M if r_rows is None else r_rows
    if fam in ("randn", "offset", "heavy"):
        a, b = torch.randn(M, KK, generator=g), torch.randn(N, KK, generator=g)
        if fam == "offset":
            a = a + 8.0
        if fam == "heavy":
            for t in (a, b):
                hit = torch.rand(t.shape, generator=g) < 4.0 / KK          # a few entries per row, times 64
                t[hit] *= 64.0
        bias, R = torch.randn(N, generator=g), torch.randn(rr, N, generator=g)
    elif fam == "exact":
        a = torch.zeros(M, KK)
        nnz = min(KK, EXACT_NNZ)
        cols = torch.rand(M, KK, generator=g).argsort(1)[:, :nnz]
        a.scatter_(1, cols, (torch.randint(0, 2, (M, nnz), generator=g) * 2 - 1).to(F32))
        b = (torch.randint(1, 3, (N, KK), generator=g) * (torch.randint(0, 2, (N, KK), generator=g) * 2 - 1)).to(F32)
        bias = torch.randint(-8, 9, (N,), generator=g).to(F32)
        R = torch.randint(-8, 9, (rr, N), generator=g).to(F32)
    elif fam == "locate":
        a = torch.zeros(M, KK)
        a[torch.arange(M), locate_column(M, KK)] = 1.0
        b = locate_code(N, KK)
        bias = torch.randint(-8, 9, (N,), generator=g).to(F32)
        R = torch.randint(-8, 9, (rr, N), generator=g).to(F32)
    else:
        raise ValueError(fam)
    a, b, bias, R = _bf(a), _bf(b), _bf(bias), _bf(R)
    d = dict(A=a[:, :K].contiguous(), B=b[:, :K].contiguous(), A2=None, B2=None, bias=bias, R=R)
    if K2:
        d["A2"], d["B2"] = a[:, K:].contiguous(), b[:, K:].contiguous()
    return d


def cancel_R(z64, r_rows, seed=0):
    """The offset family's residual for the single-rounding check: R = bf16(-z + randn), so that |z + R| is of size 1 while |z| is of size 8 sqrt(K).
    A kernel that rounds z to bf16 before adding R leaves 2^-9 |z| there, far above 2^-8 |z + R|.  (Only without r_mod: one R row per output row.)"""
    g = _gen("cancel", z64.shape[0], z64.shape[1], seed)
    return _bf((-z64 + torch.randn(z64.shape, generator=g, dtype=F64)).to(F32))[:r_rows]


def exact_holds(ref):
    """The exact family's own condition, on the reference alone: the float64 result is bit-representable in bf16."""
    return bool(torch.equal(ref.out, ref.out.to(BF16).to(F64)))


def family_tn(fam, M, I, J, seed=0):
    """P [M, I], Q [M, J], out0 [I, J] (fp32, bf16-exact P and Q).  exact: dense integers in [-3, 3]; every partial sum is an integer below 2^24 and the
    fp32 output holds it exactly.  locate: P one-hot per row m at column m % I, Q an integer code of (m, j): out[i, j] = sum of the codes of rows
    m = i (mod I), again an exact integer."""
    g = _gen("tn", fam, M, I, J, seed)
    if fam in ("randn", "offset", "heavy"):
        p, q = torch.randn(M, I, generator=g), torch.randn(M, J, generator=g)
        if fam == "offset":
            p = p + 8.0
        if fam == "heavy":
            hit = torch.rand(p.shape, generator=g) < 4.0 / I
            p[hit] *= 64.0
        o = torch.randn(I, J, generator=g)
    elif fam == "exact":
        p, q = torch.randint(-3, 4, (M, I), generator=g).to(F32), torch.randint(-3, 4, (M, J), generator=g).to(F32)
        o = torch.randint(-8, 9, (I, J), generator=g).to(F32)
    else:
        p = torch.zeros(M, I)
        p[torch.arange(M), torch.arange(M) % I] = 1.0
        m, j = torch.arange(M)[:, None], torch.arange(J)[None, :]
        q = (((5 * m + 11 * j) % 251) - 125).to(F32)
        o = torch.randint(-8, 9, (I, J), generator=g).to(F32)
    return _bf(p), _bf(q), o


# ------------------------------------------------------------------------------------------------ host emulation of the documented arithmetic
def _f(x):
    return torch.tensor(x, dtype=F32)


def act_fast32(x, act):
    """act_apply_fast of common.h in fp32: the Abramowitz-Stegun 7.1.26 erf and x * rcp(1 + exp2(c x)); rcp and exp2 as torch's fp32 ones."""
    if act == ACT_GELU:
        z = x.abs() * _f(0.70710678118654752)
        t = 1.0 / (1.0 + _f(0.3275911) * z)
        poly = t * (_f(0.254829592) + t * (_f(-0.284496736) + t * (_f(1.421413741) + t * (_f(-1.453152027) + t * _f(1.061405429)))))
        erf_abs = 1.0 - poly * torch.exp2(-z * z * _f(LOG2E))
        return _f(0.5) * x * (1.0 + torch.copysign(erf_abs, x))
    if act == ACT_QUICK_GELU:
        return x * (1.0 / (1.0 + torch.exp2(_f(-1.702) * _f(LOG2E) * x)))
    if act == ACT_SILU:
        return x * (1.0 / (1.0 + torch.exp2(_f(-LOG2E) * x)))
    return x


MUTANTS = ("drop_kstep", "k2_twice", "bias_shift", "r_row", "subtile_T", "edge_clamp", "mask_ldc", "round_before_R", "alpha_after_bias")


def emul(buf, r0, c0, A, B, A2=None, B2=None, bias=None, R=None, act=ACT_NONE, alpha=1.0, r_mod=0, remap=None, drop=None, a_drop=None, n_valid=0,
         out_bf16=True, inplace=False, mut=None):
    """Writes the emulated result into buf (a float64 host image of the output buffer; C starts at row r0, column c0) and returns it.  Arithmetic:
    fp32 products and sum, the epilogue in fp32 in the order of epilogue_store8, one rounding to bf16.  mut: one of MUTANTS."""
    A32, B32 = _c(A, F32).clone(), _c(B, F32)
    M, K = A32.shape
    N = B32.shape[0]
    if a_drop is not None:
        A32 = dropped_operand(A, a_drop[0], a_drop[1]).to(F32)
    if mut == "drop_kstep":
        A32[:, 32:64] = 0
    acc = A32 @ B32.t()
    if A2 is not None:
        seg2 = _c(A2, F32) @ _c(B2, F32).t()
        acc = acc + seg2
        if mut == "k2_twice":
            acc = acc + seg2
    if n_valid > 0:
        acc[:, 16 * ((n_valid + 15) // 16):] = 0
    b32 = None if bias is None else _c(bias, F32)
    if mut == "bias_shift" and b32 is not None:
        b32 = torch.roll(b32, 1)
    if mut == "alpha_after_bias":
        v = (acc + (0 if b32 is None else b32[None, :])) * _f(alpha)
    else:
        v = acc * _f(alpha)
        if b32 is not None:
            v = v + b32[None, :]
    v = act_fast32(v, act)
    if drop is not None:
        stride = buf.shape[1] if mut == "mask_ldc" else N
        k = keep_grid(drop[0], M, N, stride, drop[1])
        v = torch.where(k, v * _f(drop_scale(drop[1])), torch.zeros_like(v))
    rows = out_rows(M, remap)
    if R is not None or inplace:
        rr = torch.arange(M) % r_mod if r_mod > 0 else torch.arange(M)
        R32 = buf[r0:r0 + M, c0:c0 + N].to(F32) if inplace else _c(R, F32)
        if mut == "r_row":
            rr = (rr + 1) % R32.shape[0]
        if mut == "round_before_R":
            v = v.to(BF16).to(F32)
        v = v + R32[rr]
    if mut == "subtile_T" and M >= 32 and N >= 32:
        v[16:32, 16:32] = v[16:32, 16:32].t().clone()
    if out_bf16:
        v = v.to(BF16)
    v = v.to(F64)
    buf[rows + r0, c0:c0 + N] = v
    if mut == "edge_clamp":                              # the staging clamp's copy of row M - 1 stored to the next row instead of skipped
        buf[int(rows[-1]) + r0 + 1, c0:c0 + N] = v[-1]
    return buf


def emul_tn(P, Q, I, J, alpha, drop, out0):
    P32, Q32 = _c(P, F32)[:, :I], _c(Q, F32)[:, :J]
    if drop is not None:
        if tn_big_is_p(I, J):
            P32 = dropped_operand(P32, drop[0], drop[1]).to(F32)
        else:
            Q32 = dropped_operand(Q32, drop[0], drop[1]).to(F32)
    return (_c(out0, F32) + _f(alpha) * (P32.t() @ Q32)).to(F64)


# ------------------------------------------------------------------------------------------------ the one comparison both test files use
def verify(buf, r0, c0, rows, N, ref, bar):
    """buf: the whole output buffer after the call (any device, any dtype), NaN wherever nothing may be written.  rows [M] (long, on buf's device):
    the output row of each logical row.  ref [M, N] float64, bar a float64 tensor of ref's shape or 0 (then any difference counts).
    -> (canaries overwritten, elements beyond the bar, worst error / bar)."""
    b = buf.to(F64)
    written = torch.zeros(b.shape, dtype=torch.bool, device=b.device)
    written[rows + r0, c0:c0 + N] = True
    canary = int((~torch.isnan(b) & ~written).sum())
    got = b[rows + r0, c0:c0 + N]
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    if not torch.is_tensor(bar):
        over = int((err > bar).sum())
        return canary, over, float("inf") if over else 0.0
    over = int((err > bar).sum())
    return canary, over, float((err / bar.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------ geometry and epilogue tables of the GPU file
_Epi = namedtuple("Epi", "name bias R inplace r_mod remap alpha act f32 strided drop narrow")


def Epi(name, bias=False, R=False, inplace=False, r_mod=0, remap=None, alpha=1.0, act=ACT_NONE, f32=False, strided=False, drop=False, narrow=False):
    return _Epi(name, bias, R, inplace, r_mod, remap, alpha, act, f32, strided, drop, narrow)


EPIS = (
    Epi("plain"), Epi("bias", bias=True), Epi("R", R=True), Epi("bias_R", bias=True, R=True), Epi("R_inplace", R=True, inplace=True),
    Epi("rmod_remap", R=True, r_mod=13, remap=(13, 14, 1)), Epi("alpha", bias=True, alpha=0.5),
    Epi("gelu", bias=True, act=ACT_GELU), Epi("quick_gelu", bias=True, act=ACT_QUICK_GELU), Epi("silu", R=True, act=ACT_SILU),
    Epi("f32", bias=True, R=True, f32=True), Epi("f32_gelu", bias=True, act=ACT_GELU, f32=True), Epi("strided", strided=True),
    Epi("drop", R=True, drop=True), Epi("narrow", bias=True, R=True, narrow=True), Epi("narrow_gelu", bias=True, act=ACT_GELU, narrow=True),
    Epi("narrow_drop", drop=True, narrow=True, alpha=0.5),
)
LEAN = ("plain", "bias", "R", "bias_R", "R_inplace", "gelu", "quick_gelu", "silu", "strided")      # what the persistent 4-wave kernels' plan accepts
DROP_SEED = 0x5EED1234
TILE_MN = ((129, 136), (257, 264), (300, 516), (513, 520))
TILE_K = ((64, 0), (128, 0), (192, 64), (448, 64), (1024, 128))
TILED = ("128", "RING", "H16", "HP16", "W4", "WP4", "DP")
VARIANT = {"128": 0, "RING": 2, "H16": 5, "HP16": 6, "W4": 7, "WP4": 8, "DP": 9}


def drop_p(fam):
    """p = 0.5 in the zero-bar families (the scale 2 is exact), 0.05 (3276 / 65536) elsewhere."""
    return 0.5 if fam in ZERO_BAR else 0.05


def accepts(kernel, M, N, K, K2, e):
    """What av_gemm_plan's conditions say of a forced tiled kernel, restated: True = the call must be planned on `kernel`, False = it falls to 128."""
    if kernel == "128":
        return True
    if M <= 128:
        return False
    if kernel in ("W4", "WP4", "DP") and K + K2 < 128:
        return False
    if kernel in ("WP4", "DP"):
        return e.name in LEAN and N % 8 == 0 and not e.narrow
    return True


def epi_ok(fam, e):
    """Activations are not exact: the zero-bar families take the linear epilogues only."""
    return not (fam in ZERO_BAR and e.act != ACT_NONE)


SMALLM_M, SMALLM_N, SMALLM_K, SMALLM_K2 = (1, 2, 15, 16), (16, 528), (256, 512, 2304), (0, 64)
SMALLM_EPIS = (Epi("plain"), Epi("bias", bias=True), Epi("gelu", bias=True, act=ACT_GELU), Epi("silu", act=ACT_SILU, alpha=0.5),
               Epi("R_rmod", R=True, r_mod=3), Epi("f32", bias=True, R=True, f32=True), Epi("strided", strided=True))
SKINNY_M, SKINNY_K, SKINNY_NV = (15, 16, 17, 256, 257, 300), (256, 512, 2304), (0, 8, 16, 32, 33, 64)
F32_MN, F32_K, F32_K2 = ((1, 8), (65, 68), (130, 70), (64, 6)), (64, 192), (0, 64)
F32_EPIS = tuple(e for e in EPIS if not e.narrow and not e.f32)
TN_I, TN_J, TN_M = (128, 384), (1, 8, 16), (1, 63, 64, 65, 257, 1000, 16500)
PERSIST_K = (128, 192, 320)


def sample_rows(M, tile=256):
    """Rows 0, 255, 256, M - 1 and one row per tile row."""
    s = {0, min(255, M - 1), min(256, M - 1), M - 1}
    s.update(min(t * tile + (37 * t + 11) % tile, M - 1) for t in range((M + tile - 1) // tile))
    return torch.tensor(sorted(s))
