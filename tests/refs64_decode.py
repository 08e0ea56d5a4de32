"""Float64 restatement, host emulation and test inputs of avllm_dec_proj (csrc/decode.hip), the fused projection of the token step.

dec_proj64 restates the operation in float64 in the order the kernel documents: xg = bf16(x g) when the norm is folded (a product of two bf16
values is exact in fp32, so this rounding is unique), the exact sum over K against the dequantised weights, times 1 / sqrt(mean x^2 + eps), + bias,
+ scale (lt[:r] . lb[:r]), then + R | silu(gate) up | the rotation with the given table (pairs (i, i + hd/2)), and ONE rounding to the output type.
emul runs the same in fp32 in the kernel's order (8-wave deal of the 128-column groups, 32-product MFMA steps in the weight form's element order,
the partials added in wave order, the epilogue chain); MUTANTS are slips of that emulation, each wrong the way a kernel slip would be.
tests/test_decode_refs_cpu.py holds the restatement to plain torch, the emulation to the bar and every mutant over it; tests/test_decode_pin_gpu.py
runs the kernels on the same cases.  Nothing here touches the GPU library except wargs(), which uploads (and for fp8 quantises) a weight matrix."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import torch

import mxfp4_ref as mx4
from oracle import mxfp8

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
FORMS = ("bf16", "fp8", "fp4")
DW = 8                       # waves of a workgroup: the K split
PLAIN, SWIGLU, QKV = 0, 1, 2


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(shape, lo, hi, *key):
    return torch.randint(lo, hi + 1, shape, generator=gen(*key)).float()


def _bf(x):
    return x.to(BF).to(F32)


# ------------------------------------------------------------------------------------------------ weights every form holds exactly
def holds(W, form):
    """True when the weight form represents the host matrix W exactly (bf16: bf16 values; fp8 / fp4: the MX quantiser returns W)."""
    if form == "bf16":
        return torch.equal(W.to(BF).float(), W)
    if form == "fp8":
        return torch.equal(mxfp8.fake_quant(W), W)
    return torch.equal(mx4.fake_quant(W), W)


def block_exponents(W, form):
    """int32 [rows, K/32]: the E8M0 exponent the form stores for each 32-block (None for bf16)."""
    return None if form == "bf16" else (mxfp8 if form == "fp8" else mx4).block_exponents(W)


def wargs(W, form):
    """dec_proj's weight arguments for the host matrix W (values every form holds exactly) in one of the three forms."""
    from avllm import ops
    if form == "bf16":
        assert torch.equal(W.to(BF).float(), W)
        return dict(W=W.to(BF).cuda())
    if form == "fp8":
        q, e = ops.mx_quantize(W.to(BF).cuda(), 2)
        assert torch.equal(mxfp8.dequantize(q.cpu(), e.cpu().to(torch.int32) - 127), W)
        return dict(W=None, W8=q, E8=e)
    codes, e = mx4.quantize(W)
    assert torch.equal(mx4.dequantize(codes, e), W)
    return dict(W=None, W4=mx4.pack(codes).cuda(), E8=(e + 127).to(torch.uint8).cuda())


def distinct_bias(N):
    """bias[n] = n - N/2: distinct integers of magnitude <= 256, each a bf16 value."""
    assert N <= 512
    b = (torch.arange(N) - N // 2).float()
    assert torch.equal(b.to(BF).float(), b)
    return b


def rope_table(hd, cos, sin):
    return torch.tensor([cos, sin], dtype=torch.float32).repeat(hd // 2, 1).contiguous().cuda()


def rot(t, nh, hd, cos, sin):
    """apply_rotary_pos_emb with one (cos, sin) for every frequency: pairs (i, i + hd/2) inside each head."""
    M = t.shape[0]
    t = t.view(M, nh, hd)
    a, b = t[..., : hd // 2], t[..., hd // 2:]
    return torch.cat([a * cos - b * sin, b * cos + a * sin], -1).reshape(M, nh * hd)


@functools.lru_cache(maxsize=8)
def grid_weights(N, K):
    """(Cached: do not write into the result.)  Weights on the MXFP4 grid, every 32-block of a row with its own exponent (the exponents cycle over 8 values so that any K fits fp32's
    24 bits): e4m3 and bf16 hold them too, and the fp8 quantiser gives neighbouring blocks distinct exponent bytes as well."""
    W = torch.zeros(N, K)
    for b in range(K // 32):
        W[:, 32 * b:32 * b + 32] = (torch.arange(32) % 7 - 3).float() * 2.0 ** (b % 8 - 3) * (1.0 - 2.0 * (torch.arange(N) % 2)).float()[:, None]
    W[:, 1::2] *= 0.5
    return W


_LOC_VALS = torch.tensor([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])


def locate_weights(N, K):
    """W[n, k] = v(k % 32) * 2^E(n, k / 32) on the MXFP4 grid.  With k % 32 = 8 c + e the value index (e + 3 c) % 14 differs between the 8
    elements of a lane's step (a swapped nibble, byte or dword) and between the 4 chunks of 8 of a block (another step of the lane in the
    fp8 and fp4 forms); all 14 values occur in every block, so its amax is 6 and the stored exponent is E.  E = (b + n + 3 (n / 8)) % 8 - 4
    differs between neighbouring blocks (another step in the bf16 form, the neighbouring exponent byte), columns n and n ^ 8, n and n +- 1,
    n and n +- 16.  So W[n', k'] != W[n, k] for every (n', k') a slip of the kernel's index arithmetic would take in the place of (n, k)."""
    k = torch.arange(K)
    idx = k % 32
    v = _LOC_VALS[((idx % 8) + 3 * (idx // 8)) % 14]
    n = torch.arange(N)[:, None]
    E = ((k // 32)[None, :] + n + 3 * (n // 8)) % 8 - 4
    return v[None, :] * torch.ldexp(torch.ones(()), E.to(torch.int32))


def step_norm(K, lo=0):
    """Norm weights 2^(lo + ((k / 8) + (k / 32)) % 4): powers of two (the fold x g stays exact) that differ between step j and step j + 1 of a
    lane in every weight form (bf16: k + 32; fp4: k + 8; fp8: k + 8 inside a 64-column pair, k + 56 to the next)."""
    k = torch.arange(K)
    return torch.ldexp(torch.ones(()), (lo + ((k // 8) + (k // 32)) % 4).to(torch.int32))


# ------------------------------------------------------------------------------------------------ the float64 restatement
def _d(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu").to(F64)


def rot_index(N, dq, dkv, hd):
    """Per logical column of [q | k | v]: (partner column, index into the table, sign of the sine term); v columns: (itself, -1, 0)."""
    n = torch.arange(N)
    half = hd // 2
    i = n % hd
    first = i < half
    partner = torch.where(first, n + half, n - half)
    sign = torch.where(first, -1.0, 1.0).to(F64)
    ti = i % half
    v = n >= dq + dkv
    return torch.where(v, n, partner), torch.where(v, -1, ti), torch.where(v, torch.zeros((), dtype=F64), sign)


def dec_proj64(A, W, mode=PLAIN, g=None, eps=1e-5, R=None, bias=None, lt=None, lbs=None, r=0, scale=0.0, dq=0, dkv=0, hd=0, rope=None,
               out_f32=False):
    """-> namespace: out [M, N out] float64 (mode 2: the logical [q | k | v] columns; k and v are the cache rows at pos + *pos_dev), rounded = out
    after the ONE rounding to the output type, and what bars.dec_proj_bar needs: acc (exact sum), sum_abs, rstd, y, zb, u, u_abs, z, cosv, sinv,
    partner.  A [M, K], g [K], R [M, N], bias [N]: bf16 values; W [rows, K] dequantised weights; lt [M, >= 64 nmod] f32; lbs: B images
    [rows of module j, >= r]; rope [hd/2, 2] f32 (cos, sin)."""
    A_, W_, g_ = _d(A), _d(W), _d(g)
    K = A_.shape[1]
    xg = A_ if g is None else (A_ * g_[None, :]).to(F32).to(BF).to(F64)           # exact in fp32, so float64 -> fp32 -> bf16 rounds once
    acc = xg @ W_.t()
    sa = xg.abs() @ W_.abs().t()
    rstd = None if g is None else torch.rsqrt((A_ * A_).mean(-1, keepdim=True) + eps)
    y = acc if g is None else acc * rstd
    zb = y if bias is None else y + _d(bias)[None, :]
    u = u_abs = None
    z = zb
    if lt is not None:
        lt_ = _d(lt)
        u = torch.cat([lt_[:, 64 * j:64 * j + r] @ _d(lb)[:, :r].t() for j, lb in enumerate(lbs)], 1)
        u_abs = torch.cat([lt_[:, 64 * j:64 * j + r].abs() @ _d(lb)[:, :r].abs().t() for j, lb in enumerate(lbs)], 1)
        z = zb + scale * u
    ref = SimpleNamespace(mode=mode, K=K, acc=acc, sum_abs=sa, rstd=rstd, y=y, zb=zb, u=u, u_abs=u_abs, scale=scale, z=z, R=_d(R), bias=bias is not None,
                          out_f32=out_f32, x_sq=(A_ * A_).sum(-1, keepdim=True))
    if mode == PLAIN:
        out = z if R is None else z + ref.R
    elif mode == SWIGLU:
        F = W_.shape[0] // 2
        ref.F = F
        gate, up = z[:, :F], z[:, F:]
        out = gate * torch.sigmoid(gate) * up
    else:
        N = W_.shape[0]
        partner, ti, sign = rot_index(N, dq, dkv, hd)
        tab = _d(rope)
        ref.cosv = torch.where(ti >= 0, tab[ti.clamp_min(0), 0], torch.ones((), dtype=F64))
        ref.sinv = sign * tab[ti.clamp_min(0), 1]
        ref.partner = partner
        out = z * ref.cosv[None, :] + z[:, partner] * ref.sinv[None, :]
    ref.out = out
    ref.rounded = out.to(F32).to(F64) if out_f32 else out.to(F32).to(BF).to(F64)
    return ref


# ------------------------------------------------------------------------------------------------ the K deal, the ring and the step order
def deal(K):
    """[(k0, G)] of the 8 waves: U = K / 128 groups, wave w gets ub = U / 8 of them and one more while w < ue = U % 8, from column k0."""
    U = K // 128
    ub, ue = U // DW, U % DW
    return [(128 * (w * ub + min(w, ue)), ub + (1 if w < ue else 0)) for w in range(DW)]


def al_of(M):
    return 1 if M <= 4 else 2 if M <= 8 else 4


def depth(form, al):
    """Ring depth D (DecForm::depth): groups a wave keeps in flight."""
    return (3 if al == 4 else 4) if form == "fp4" else 2


def ring_path(G, D):
    """(trips of the main loop, groups left to the straight-line tail) of a wave with G groups: `for (g = 0; g + 2 D <= G; g += D)`."""
    trips = 0
    g = 0
    while g + 2 * D <= G:
        g += D
        trips += 1
    return trips, G - g


def step_cols(form, j):
    """The 32 column offsets inside a 128-column group that MFMA step j multiplies, in (fq, e) order (DecForm::koff)."""
    fq, e = np.repeat(np.arange(4), 8), np.tile(np.arange(8), 4)
    if form == "bf16":
        return 32 * j + 8 * fq + e
    if form == "fp8":
        return 64 * (j >> 1) + 16 * fq + 8 * (j & 1) + e
    return 32 * fq + 8 * j + e


# ------------------------------------------------------------------------------------------------ host emulation in fp32, kernel order
MUTANTS = ("drop_last_group", "k0_overlap", "exp_neighbour", "nibble_swap", "norm_next_step", "al_rotate", "rstd_before_round", "gate_up_swapped",
           "rot_sign_flip", "rot_index_mask", "bias_after_rot", "lora_after_rot", "bias_lora_after_rot", "lora_module_off", "r_after_round")
# the default emulation takes the rotary index as col % (hd / 2); "rot_index_mask" takes (col % hd) & (hd / 2 - 1), the kernel's expression, which is
# the same for a power of two and wrong otherwise (hd = 96: column 16 takes angle 0) -- the reason the host check refuses such head dims.

f32 = np.float32


def _np(t):
    return None if t is None else torch.as_tensor(t).detach().to("cpu").to(F64).numpy()


def _to_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF).to(F32).numpy()


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def emul(A, W, form, mode=PLAIN, g=None, eps=1e-5, R=None, bias=None, lt=None, lbs=None, r=0, scale=0.0, dq=0, dkv=0, hd=0, rope=None,
         out_f32=False, mutant=None):
    """The kernel's arithmetic on the host -> [M, N out] float64 holding the rounded outputs, columns as dec_proj64's."""
    assert mutant is None or mutant in MUTANTS
    A_ = _np(A).astype(f32)
    Wm = _np(W).astype(f32).copy()
    M, K = A_.shape
    rows = Wm.shape[0]
    if mutant == "exp_neighbour" and form != "bf16":             # block b scaled by the exponent byte of block b ^ 1
        e = block_exponents(torch.from_numpy(Wm), form).numpy()
        sw = e.reshape(rows, -1, 2)[:, :, ::-1].reshape(rows, -1)
        Wm = (Wm.reshape(rows, -1, 32) * np.exp2((sw - e).astype(np.float64))[:, :, None]).reshape(rows, K).astype(f32)
    if mutant == "nibble_swap" and form == "fp4":                # elements 2 i and 2 i + 1 of a byte exchanged
        Wm = Wm.reshape(rows, K // 2, 2)[:, :, ::-1].reshape(rows, K).copy()
    dl = deal(K)
    if mutant == "drop_last_group":
        w_ = max(w for w in range(DW) if dl[w][1] > 0)
        dl[w_] = (dl[w_][0], dl[w_][1] - 1)
    if mutant == "k0_overlap":
        w_ = max(w for w in range(DW) if dl[w][1] > 0)
        if w_ > 0:
            dl[w_] = (dl[w_][0] - 128, dl[w_][1])
    norm = g is not None
    # columns permuted so that group `grp`, step j is the contiguous slice [128 grp + 32 j, + 32) in (fq, e) order
    perm = (128 * np.arange(K // 128)[:, None, None] + np.stack([step_cols(form, j) for j in range(4)])[None]).reshape(-1)
    X = A_[:, perm].reshape(M, K // 128, 4, 32)
    Wp = Wm[:, perm].astype(np.float64).reshape(rows, K // 128, 4, 32)
    maxG = max(G for _, G in dl)
    # RMS statistics: lane (m, fq) adds its 8 squares per step in order; fq partials meet by two butterflies, waves in order
    rstd = None
    if norm:
        sq = (X.astype(np.float64) ** 2).astype(f32).reshape(M, K // 128, 4, 4, 8).transpose(0, 3, 1, 2, 4).reshape(M, 4, K // 128, 32)
        chain = np.zeros((DW, M, 4, maxG * 32), f32)
        for w, (k0, G) in enumerate(dl):
            chain[w, :, :, :G * 32] = sq[:, :, k0 // 128:k0 // 128 + G].reshape(M, 4, G * 32)
        ss = np.zeros((DW, M, 4), f32)
        for i in range(maxG * 32):
            ss = ss + chain[..., i]                              # x * x of two bf16 values is exact in fp32: an fma and a product + sum agree
        sw = (ss[..., 0] + ss[..., 1]) + (ss[..., 2] + ss[..., 3])
        t = np.zeros((M,), f32)
        for w in range(DW):
            t = t + sw[w]
        rstd = (f32(1.0) / np.sqrt(t / f32(K) + f32(eps))).astype(f32)[:, None]
        gp = _np(g).astype(f32)[perm].reshape(K // 128, 4, 32)
        if mutant == "norm_next_step":
            gp = np.roll(gp, -1, axis=1)
    if mutant == "al_rotate" and M > 8:                          # rows >= 8 take the activations of the step before (inside the group)
        X = X.copy()
        X[8:] = np.roll(X[8:], 1, axis=2)
    if norm:
        if mutant == "rstd_before_round":
            X = _to_bf16((X * rstd[:, :, None, None]).astype(f32) * gp[None])
        else:
            X = _to_bf16(X * gp[None])
    prod = np.einsum("mgjk,ngjk->gjmn", X.astype(np.float64), Wp)              # one MFMA step each: 32 exact products, summed in float64
    steps = np.zeros((DW, maxG * 4, M, rows))
    for w, (k0, G) in enumerate(dl):
        steps[w, :G * 4] = prod[k0 // 128:k0 // 128 + G].reshape(G * 4, M, rows)
    part = np.zeros((DW, M, rows), f32)
    for i in range(maxG * 4):
        part = (part.astype(np.float64) + steps[:, i]).astype(f32)
    acc = np.zeros((M, rows), f32)
    for w in range(DW):
        acc = acc + part[w]
    s = acc
    if norm and mutant != "rstd_before_round":
        s = s * rstd
    bv = None if bias is None else _np(bias).astype(f32)[None, :]
    late_bias = mutant in ("bias_after_rot", "bias_lora_after_rot") and mode == QKV
    late_lora = mutant in ("lora_after_rot", "bias_lora_after_rot") and mode == QKV
    if bv is not None and not late_bias:
        s = s + bv
    lterm = None
    if lt is not None:
        lt_ = _np(lt).astype(f32)
        us = []
        nmod = len(lbs)
        for j, lb in enumerate(lbs):
            lb_ = _np(lb).astype(f32)
            jj = (j + 1) % nmod if mutant == "lora_module_off" else j
            u = np.zeros((M, lb_.shape[0]), f32)
            for i in range(r):
                u = _fma(lt_[:, 64 * jj + i][:, None], lb_[:, i][None, :], u)
            us.append(u)
        lterm = (f32(scale) * np.concatenate(us, 1)).astype(f32)
        if not late_lora:
            s = s + lterm
    if mode == PLAIN:
        if R is not None:
            R_ = _np(R).astype(f32)
            s = _to_bf16(s) + R_ if mutant == "r_after_round" else s + R_
        o = s
    elif mode == SWIGLU:
        F = rows // 2
        gate, up = (s[:, F:], s[:, :F]) if mutant == "gate_up_swapped" else (s[:, :F], s[:, F:])
        with np.errstate(over="ignore"):
            o = (gate / (f32(1.0) + np.exp(-gate).astype(f32))).astype(f32) * up
    else:
        n = np.arange(rows)
        half = hd // 2
        i = n % hd
        first = i < half
        partner = np.where(first, n + half, n - half)
        ti = (i & (half - 1)) if mutant == "rot_index_mask" else i % half
        tab = _np(rope).astype(f32)
        c, sn = tab[ti, 0][None, :], tab[ti, 1][None, :]
        rotary = n < dq + dkv
        other = s[:, np.where(rotary, partner, n)]
        sign = np.where(first, f32(-1.0), f32(1.0))
        if mutant == "rot_sign_flip":
            sign = np.full_like(sign, f32(-1.0))
        o = np.where(rotary[None, :], (s * c).astype(f32) + (sign[None, :] * (other * sn).astype(f32)), s).astype(f32)
        if late_bias and bv is not None:
            o = o + bv
        if late_lora and lterm is not None:
            o = o + lterm
    o = o.astype(f32)
    return torch.from_numpy(o if out_f32 else _to_bf16(o)).to(F64)


# ------------------------------------------------------------------------------------------------ the cases both test files run
K_DEAL = (128, 384, 2560, 4608, 6656, 8704, 11008)          # U = 1, 3, 20, 36, 52, 68, 86: 0 .. 11 groups per wave
M_DEAL = (1, 4, 5, 8, 9, 16)                                # both sides of the activation-load forms' boundaries
N_PLAIN = 48                                                # three workgroups
VARIANTS = ("plain", "norm", "norm_R")
FAMILIES = ("exact", "randn", "offset", "heavy")
EPS = 1e-5


@functools.lru_cache(maxsize=8)
def mx_weights(rows, K, *key, heavy=False):
    """(Cached: do not write into the result.)  Gaussian weights of size K^-1/2 rounded onto the MXFP4 grid: values all three forms hold."""
    w = torch.randn(rows, K, generator=gen("w", rows, K, *key)) * K ** -0.5
    if "offset" in key:                                   # offset: a mean of one sigma, so that |z| is of the size of sum_abs (8 sqrt K) at every K
        w = w + K ** -0.5
    if heavy:
        hit = torch.rand(w.shape, generator=gen("wh", rows, K, *key)) < 4.0 / K
        w[hit] *= 64.0
    return mx4.fake_quant(w)


def acts(fam, M, K, *key):
    a = torch.randn(M, K, generator=gen("a", fam, M, K, *key))
    if fam == "offset":
        a = a + 8.0
    if fam == "heavy":
        hit = torch.rand(a.shape, generator=gen("ah", M, K, *key)) < 4.0 / K
        a[hit] *= 64.0
    return _bf(a)


def rand_norm(K, *key):
    return _bf(1.0 + 0.1 * torch.randn(K, generator=gen("g", K, *key)))


def plain_case(fam, variant, M, K, N=N_PLAIN):
    """One mode-0 launch: kwargs of dec_proj64 / emul (host tensors), `exact` = the accumulator carries the bar 0."""
    norm, res = variant != "plain", variant == "norm_R"
    c = dict(mode=PLAIN, eps=EPS, out_f32=True)
    if fam == "exact":
        c["A"], c["W"] = ints((M, K), -2, 2, "xa", M, K), grid_weights(N, K)
        if norm:
            c["g"] = step_norm(K) % 3.0                      # 1, 2, 1, 2: integer powers of two, the fold stays exact and the sums small
        if res:
            c["R"] = ints((M, N), -5, 5, "xr", M)
    else:
        c["A"], c["W"] = acts(fam, M, K), mx_weights(N, K, fam, heavy=fam == "heavy")
        c["out_f32"] = fam == "randn"                        # the other two: bf16 output, the ONE rounding
        if norm:
            c["g"] = rand_norm(K)
        if res:
            z = dec_proj64(**c).z
            c["R"] = _bf((-z + torch.randn(z.shape, generator=gen("rr", fam, M, K), dtype=F64)).float()) if fam == "offset" else \
                _bf(torch.randn(M, N, generator=gen("rn", fam, M, K)))
    return c


def locate_groups(K):
    """Groups (units of 128 columns) the locate family walks: the first, a middle and the last group, which lie in different waves for U >= 3."""
    U = K // 128
    return sorted({0, U // 2, U - 1})


def locate_acts(M, K, grp):
    """[L, M, K]: row m of launch l is hot (1.0) at k = 128 grp + M l + m, L = ceil(128 / M) launches cover the group (M = 16: k = 128 g + 16 l + m)."""
    L = -(-128 // M)
    A = torch.zeros(L, M, K)
    hot = torch.full((L, M), -1, dtype=torch.int64)
    for l in range(L):
        for m in range(M):
            if M * l + m < 128:
                hot[l, m] = 128 * grp + M * l + m
                A[l, m, hot[l, m]] = 1.0
    return A, hot


def locate_expect(W, hot, g=None):
    """[L, M, N] float64: the weight (times the norm weight) at the hot column, 0 for a row that has none; before rstd."""
    Wd = W.double()
    col = Wd.t()[hot.clamp_min(0)]                                     # [L, M, N]
    if g is not None:
        col = col * g.double()[hot.clamp_min(0)][..., None]
    return col * (hot >= 0).double()[..., None]


def name_of(W, g, value, grp):
    """The (n, k) of group `grp` whose weight (times norm weight) is nearest `value`: what a wrong locate output actually multiplied."""
    Wg = W[:, 128 * grp:128 * grp + 128].double() * (1.0 if g is None else g[128 * grp:128 * grp + 128].double()[None, :])
    d = (Wg - value).abs()
    return [(n, 128 * grp + k) for n, k in (d <= d.min() + 1e-3 * abs(value)).nonzero()[:4].tolist()]


def locate_check(run, K, Ms=M_DEAL, N=N_PLAIN):
    """The locate family over `run(A [L, M, K], norm) -> [L, M, N] float64` (the kernel, or the emulation): bar 0 without the norm, the rstd terms
    alone with it.  Raises with the (n, k) that was multiplied in the place of the expected one; returns the worst err / bar of the normed launches."""
    import bars
    W, g = locate_weights(N, K), step_norm(K)
    worst = 0.0
    for M in Ms:
        for grp in locate_groups(K):
            A, hot = locate_acts(M, K, grp)
            for norm in (False, True):
                got = run(A, norm)
                want = locate_expect(W, hot, g if norm else None)
                rstd = None
                if not norm:
                    ok = got == want
                else:
                    rstd = torch.rsqrt(torch.tensor(1.0 / K + EPS, dtype=F64)) * (hot >= 0).double()[..., None]
                    want = want * rstd
                    ref = SimpleNamespace(mode=PLAIN, K=K, acc=want, sum_abs=want.abs(), rstd=rstd, y=want, zb=want, z=want, u=None, bias=False, R=None,
                                          out=want, out_f32=True)
                    bar = bars.dec_proj_bar(ref, exact=True)
                    err = (got - want).abs()
                    ok = err <= bar
                    worst = max(worst, float((err / bar).max()))
                if not bool(ok.all()):
                    l, m, n = (~ok).nonzero()[0].tolist()
                    v = float(got[l, m, n]) / ((float(rstd[l, m, 0]) or 1.0) if norm else 1.0)
                    raise AssertionError(f"M={M} group {grp} norm={norm}: row {m} of launch {l}, column {n}, hot k={int(hot[l, m])}: got {float(got[l, m, n])!r}, "
                                         f"want {float(want[l, m, n])!r}; the weight nearest to what came out sits at (n, k) in "
                                         f"{name_of(W, g if norm else None, v, grp)}")
    return worst


def swiglu_case(fam, M, K, F):
    """Mode 1: W = [gate; up] of F columns each, norm folded (the model's launch).  randn: gate weights scaled so that the pre-activations reach
    +-20; locate: zero gate weights are not possible without a bias, so the gate rows are equal (one constant per row m) and up = a distinct
    integer per column."""
    c = dict(mode=SWIGLU, eps=EPS, out_f32=False)
    if fam == "locate":
        A = torch.zeros(M, K)
        A[:, 0] = 1.0 + torch.arange(M).float() % 4                    # x = (1 + m % 4) e_0: rstd = sqrt(K) / x_0 up to eps, gate = w_g sqrt(K) for every m
        W = torch.zeros(2 * F, K)
        W[:F, 0] = 0.5                                                 # gate: one constant for all columns
        W[F:, 0] = _LOC_VALS[torch.arange(F) % 14] * 8.0 ** (torch.arange(F) // 14)               # up: distinct per column (F <= 42), one grid value per block
        c["A"], c["W"], c["g"] = A, W, torch.ones(K)
        return c
    W = mx_weights(2 * F, K, "sw", F).clone()
    A = acts("randn", M, K, "sw", F)
    c["A"], c["W"], c["g"] = A, W, rand_norm(K, "sw")
    z = dec_proj64(**c).z[:, :F]
    amp = 20.0 / float(z.abs().max())
    amp = 2.0 ** round(float(np.log2(amp)))                            # a power of two keeps the values on the grid
    W[:F] *= amp
    return c


def real_rope(hd, pos, theta=10000.0):
    """[hd/2, 2] fp32 (cos, sin) of HF's fp32 angle pos * inv_freq_i."""
    inv = 1.0 / (torch.tensor(theta, dtype=F32) ** (torch.arange(0, hd, 2, dtype=torch.int64).to(F32) / hd))
    ang = (torch.tensor(float(pos), dtype=F32) * inv).to(F64)
    return torch.stack([ang.cos(), ang.sin()], -1).to(F32).contiguous()


ROPE_POS = 1000          # cos and sin take all four sign pairs over the frequencies of hd = 32, 64 and 128 (asserted by qkv_case)


def qkv_case(fam, M, K, hd, heads, kvh, lora, bias=False):
    """Mode 2 with the norm folded and real angles; adapters on all three modules when `lora`."""
    dq, dkv = heads * hd, kvh * hd
    N = dq + 2 * dkv
    tab = real_rope(hd, ROPE_POS)
    signs = {(bool(c > 0), bool(s > 0)) for c, s in tab.tolist()}
    assert len(signs) == 4 or hd & (hd - 1)
    c = dict(mode=QKV, eps=EPS, out_f32=False, dq=dq, dkv=dkv, hd=hd, rope=tab)
    if fam == "exact":
        c["A"], c["W"], c["g"] = ints((M, K), -2, 2, "qa", M, K), grid_weights(N, K), torch.ones(K)
    else:
        c["A"], c["W"], c["g"] = acts(fam, M, K, "q", hd), mx_weights(N, K, "q", hd, heads), rand_norm(K, "q")
    if bias:
        c["bias"] = _bf(4.0 * torch.randn(N, generator=gen("qb", N)))
    if lora:
        r = 8
        lt = torch.zeros(M, 200)                                       # ld_lora_t 200 > 64 * 3
        lbs = []
        for j, w in enumerate((dq, dkv, dkv)):
            lt[:, 64 * j:64 * j + r] = torch.randn(M, r, generator=gen("lt", j, M)) * (1.0 + j)
            lb = torch.zeros(w, 64)
            lb[:, :r] = _bf(torch.randn(w, r, generator=gen("lb", j, w)))
            lbs.append(lb)
        c.update(lt=lt, lbs=lbs, r=r, scale=0.5)
    return c


def premise_exact(ref, unit=2.0 ** -4):
    """The exact family's premise on the reference alone: every partial sum is a multiple of `unit` below 2^24 units, so fp32 holds it in any order."""
    return float(ref.sum_abs.max()) < 2.0 ** 24 * unit and bool(torch.equal(ref.acc, (ref.acc / unit).round() * unit))


# ------------------------------------------------------------------------------------------------ the lists of cases (GPU file and CPU file alike)
SWIGLU_F, SWIGLU_K, SWIGLU_M = (8, 40), (128, 2560, 11008), (1, 8, 16)
QKV_HD, QKV_HEADS, QKV_K, QKV_M = (32, 64, 128), ((4, 2), (3, 3), (2, 1)), (128, 2560), (1, 5, 16)
QKV_SIDE = ((False, False), (True, False), (True, True))           # (adapters, bias)


def plain_cases(K):
    """-> (id, case, exact) of every mode-0 launch at this K: M x variant x family.  A case is host tensors of values every weight form holds, so
    the same list serves the three forms."""
    for M in M_DEAL:
        for variant in VARIANTS:
            for fam in FAMILIES:
                yield f"{fam}-{variant}-M{M}", plain_case(fam, variant, M, K), fam == "exact"


def swiglu_cases(F, K):
    for M in SWIGLU_M:
        for fam in ("randn", "locate"):
            yield f"{fam}-M{M}", swiglu_case(fam, M, K, F), fam == "locate"


def qkv_cases(hd, heads, kvh, K):
    for M in QKV_M:
        for lora, bias in QKV_SIDE:
            yield f"M{M}-lora{int(lora)}-bias{int(bias)}", qkv_case("randn", M, K, hd, heads, kvh, lora, bias), False
