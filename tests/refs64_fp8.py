"""Plain float64 restatements of the block-scaled fp8 family (csrc/fp8.hip, fp8_fast.hip: avllm_mx_quantize, avllm_gemm_f8, avllm_norm_mxq), the
host side of the scale image, the input families and the quantised-output rules of tests/test_fp8_pin_gpu.py.

An MX operand is a pair (codes uint8 [R, K] e4m3fn, exponents int [R, K / 32]); decode() is its exact value.  gemm_f8() is the whole formula of
avllm_gemm_f8, act(A B^T + bias) + R, in float64 from the DECODED operands, as a refs64_gemm.Ref, so bars.gemm_bar applies to it as written.
The zero-bar families are built as codes and exponents directly (never through the quantiser under test) and fed to the kernel through
encode_image(); the barred families are quantised by the device and referenced from the codes it produced (read_image()).  Nothing here
touches the GPU."""
import functools

import torch

import refs64_gemm as G
from oracle import mxfp8 as MX

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
BLOCK = 32
E4M3_MAX = 448.0
E4M3_MIN_STEP = 2.0 ** -9          # spacing of the e4m3 subnormals (below 2^-6)


# ------------------------------------------------------------------------------------------------ the element format
def _e4m3_table():
    """All 256 e4m3fn codes from the format's definition (OCP 8-bit floating point, E4M3: bias 7, no infinities, S.1111.111 = NaN)."""
    t = torch.empty(256, dtype=F64)
    for c in range(256):
        s, ex, m = c >> 7, (c >> 3) & 15, c & 7
        if ex == 15 and m == 7:
            v = float("nan")
        elif ex == 0:
            v = m * 2.0 ** -9
        else:
            v = (1 + m / 8.0) * 2.0 ** (ex - 7)
        t[c] = -v if s else v
    return t


E4M3 = _e4m3_table()


def pow2(e):
    """2^e, exact, float64, on e's device; e an integer tensor (|e| <= 1022)."""
    return torch.ldexp(torch.ones((), dtype=F64, device=e.device), e.to(torch.int32))


def decode(codes, exps):
    """codes uint8 [R, K], exps int [R, K / 32] -> float64 [R, K] on their device: table value times 2^e, exact."""
    v = E4M3.to(codes.device)[codes.long()]
    return v * pow2(exps.to(codes.device)).repeat_interleave(BLOCK, dim=-1)


def code_of(value):
    """The e4m3 code of an exactly representable value (a number or tensor)."""
    v = torch.as_tensor(value, dtype=F32)
    c = v.to(torch.float8_e4m3fn)
    assert torch.equal(c.float(), v), "not an e4m3 value"
    return c.view(torch.uint8)


# ------------------------------------------------------------------------------------------------ the scale image, host side
def image_bytes(layout, R, K):
    return R * (K // BLOCK) if layout == 2 else (K // 128) * ((R + 255) // 256 * 4) * 4 * 16 * 4


def _flat_index(layout, R, K):
    if layout == 2:
        return torch.arange(R * (K // BLOCK)).reshape(R, K // BLOCK)
    word, byte = MX.scale_image_index(layout, R, K)
    return word * 4 + byte


def encode_image(exps, layout, R, K):
    """exps int [R, K / 32] -> the whole scale image avllm_gemm_f8 / avllm_dec_proj read (uint8, avllm_mx_scale_bytes(R, K) bytes; layout 2: the plain
    [R, K / 32] matrix): E8M0 bytes e + 127 where oracle.mxfp8.scale_image_index puts them, every other byte 0."""
    img = torch.zeros(image_bytes(layout, R, K), dtype=torch.uint8)
    img[_flat_index(layout, R, K).reshape(-1)] = (exps.cpu().reshape(-1) + 127).to(torch.uint8)
    return img


def read_image(img, layout, R, K):
    """-> (exps int32 [R, K / 32], the bytes of the image that belong to no (row, block): rows >= R of a partly filled group and the groups that pad
    the image to a 256-row tile).  The second must be all zero."""
    img = img.cpu().reshape(-1)
    assert img.numel() == image_bytes(layout, R, K), (img.numel(), image_bytes(layout, R, K))
    idx = _flat_index(layout, R, K)
    used = torch.zeros(img.numel(), dtype=torch.bool)
    used[idx.reshape(-1)] = True
    assert int(used.sum()) == idx.numel(), "two (row, block) pairs share a byte"
    return img[idx.reshape(-1)].reshape(idx.shape).to(torch.int32) - 127, img[~used]


def header_image(exps, layout, R, K):
    """The same image by the index arithmetic of the header comment of csrc/fp8.hip, written out as loops: for K-step t, 64-row group rb, K-block fq,
    lane row fr: word ((t RB + rb) 4 + fq) 16 + fr, byte i = exponent of row row_of(layout, rb, i, fr), K-block 4 t + fq."""
    RB = (R + 255) // 256 * 4
    img = torch.zeros(image_bytes(layout, R, K), dtype=torch.uint8)
    for t in range(K // 128):
        for rb in range(RB):
            for fq in range(4):
                for fr in range(16):
                    for i in range(4):
                        if layout == 0:
                            row = 64 * rb + 16 * i + fr
                        else:
                            j = 4 * (rb & 1) + i
                            row = 128 * (rb >> 1) + 32 * (j >> 1) + 4 * (j & 1) + 8 * (fr >> 2) + (fr & 3)
                        if row < R:
                            img[(((t * RB + rb) * 4 + fq) * 16 + fr) * 4 + i] = int(exps[row, 4 * t + fq]) + 127
    return img


# ------------------------------------------------------------------------------------------------ the GEMM
def gemm_f8(Aq, Ae, Bq, Be, bias=None, R=None, act=G.ACT_NONE):
    """-> refs64_gemm.Ref (out, sum_abs, z, acc, rows, mask=None) of act(decode(A) decode(B)^T + bias) + R in float64."""
    return G.gemm(decode(Aq, Ae), decode(Bq, Be), bias=bias, R=R, act=act)


# ------------------------------------------------------------------------------------------------ what the scaled MFMA drops inside a group of 8 products
MFMA_GROUP, MFMA_KEEP = 8, 13          # bars.py, "block-scaled fp8 against float64": the measurement and the derivation


def code_exponent(codes):
    """The exponent the matrix pipe aligns an e4m3 operand by: field - 7, the subnormals (field 0) sharing the smallest normal binade's -6."""
    return ((codes.to(torch.int32) >> 3) & 15).clamp_min(1) - 7


def mfma_group_loss(Aq, Ae, Bq, Be):
    """-> float64 [M, N], on the operands' device: the most v_mfma_scale_f32_16x16x128_f8f6f4 can lose of sum_k a_k b_k by its alignment INSIDE each group
    of 8 consecutive k.  With E_g the largest exponent sum ex(a_k) + ex(b_k) among the group's non-zero products, every product is cut towards zero to
    a multiple of 2^(E_g - 13) (times the two block scales, which a group shares): it loses |a_k b_k| mod that, exactly, which is 0 for a product
    whose exponent sum is within 7 of E_g (8 significant bits).  The sum of these over k bounds the error (the signs of the products may cancel it)."""
    dev = Aq.device
    M, K = Aq.shape
    N = Bq.shape[0]
    a, b = decode(Aq, Ae).abs(), decode(Bq, Be.to(Bq.device)).abs()
    xa = code_exponent(Aq) + Ae.to(dev).to(torch.int32).repeat_interleave(BLOCK, dim=-1)
    xb = code_exponent(Bq) + Be.to(dev).to(torch.int32).repeat_interleave(BLOCK, dim=-1)
    xa = torch.where(a > 0, xa, torch.full_like(xa, -100000))          # a zero operand sets no exponent
    xb = torch.where(b > 0, xb, torch.full_like(xb, -100000))
    loss = torch.zeros(M, N, dtype=F64, device=dev)
    for g in range(K // MFMA_GROUP):
        sl = slice(MFMA_GROUP * g, MFMA_GROUP * (g + 1))
        E = xa[:, None, sl] + xb[None, :, sl]
        p = a[:, None, sl] * b[None, :, sl]
        Eg = E.amax(-1, keepdim=True)
        cut = pow2((Eg - MFMA_KEEP).clamp_min(-1000))
        loss += torch.fmod(p, cut).sum(-1)
    return loss


# ------------------------------------------------------------------------------------------------ the MX rule on float64 values
def block_exp(amax):
    """e = floor(log2 amax) - 8 clamped to [-127, 127]; amax == 0 (or below 2^-119, where the clamp holds) -> -127.  amax float64 >= 0."""
    _, ex = torch.frexp(amax.clamp_min(2.0 ** -300))           # amax = m 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    return (ex - 1 - 8).clamp(-127, 127).to(torch.int32)


def admissible_exps(ref, bar):
    """ref, bar float64 [R, N] (bar a tensor or a number) -> (lo, hi) int32 [R, N / 32]: every exponent the rule can give a block whose elements lie
    within bar of ref.  Its maximum then lies in [max (|ref| - bar), max (|ref| + bar)], and the exponent is monotone in the maximum."""
    a = ref.abs().reshape(ref.shape[0], -1, BLOCK)
    b = bar.reshape(a.shape) if torch.is_tensor(bar) else bar
    return block_exp((a - b).clamp_min(0.0).amax(-1)), block_exp((a + b).amax(-1))


def e4m3_step(s):
    """Spacing of the e4m3 values around the scaled magnitude s >= 0 (float64): 2^-9 in the subnormal range (below 2^-6), 2^(floor(log2 s) - 3) up to
    the top binade [256, 448], whose 32 also holds above (the clamp is the caller's exception)."""
    _, ex = torch.frexp(s.clamp(2.0 ** -6, 256.0))
    return pow2(ex - 1 - 3)


def codes_at(x, e):
    """The rule's elements of x (float64 [R, N], rounded to fp32 first: the device quantises fp32 values) under GIVEN block exponents e [R, N / 32]:
    RNE(x 2^-e) saturated to +-448, as uint8 codes.  Monotone in x for a fixed e, which the "can move" sets below rely on."""
    s = torch.ldexp(torch.ones((), dtype=F32, device=e.device), -e.to(torch.int32)).repeat_interleave(BLOCK, dim=-1)
    return (x.to(F32) * s).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def quant_errors(codes, exps, ref, bar):
    """The two checks of a quantised result (codes uint8 [R, N], exps int [R, N / 32]: the KERNEL's) against the float64 ref under the elementwise
    bar, for every block and element: -> (blocks whose exponent lies outside the admissible set, elements beyond the half-step bound, worst
    ratio of an element's error to its bound).  The bound, in the kernel's own scale 2^e: step / 2 + bar with step = the e4m3 spacing at
    (|ref| + bar) 2^-e, subnormal range included; where that magnitude passes 448 the element may have been clamped to 448, which is worth
    max(step / 2, magnitude - 448)."""
    exps = exps.to(ref.device).to(torch.int32)
    lo, hi = admissible_exps(ref, bar)
    bad_blocks = int(((exps < lo) | (exps > hi)).sum())
    scale = pow2(exps).repeat_interleave(BLOCK, dim=-1)
    bar_t = bar if torch.is_tensor(bar) else torch.full_like(ref, float(bar))
    s = (ref.abs() + bar_t) / scale
    half = 0.5 * e4m3_step(s)
    half = torch.where(s > E4M3_MAX, torch.maximum(half, s - E4M3_MAX), half)
    bound = half * scale + bar_t
    err = (decode(codes, exps) - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    return bad_blocks, int((err > bound).sum()), float((err / bound.clamp_min(1e-300)).max())


def can_move(ref, bar):
    """From the reference and the bar alone: (blocks [R, N / 32] whose admissible set holds more than one exponent, elements [R, N] whose code is not
    the same at ref - bar and ref + bar under the block's one exponent, or that sit in such a block).  Outside both sets codes and exponents must
    EQUAL the rule applied to ref."""
    lo, hi = admissible_exps(ref, bar)
    blk = lo != hi
    el = (codes_at(ref - bar, lo) != codes_at(ref + bar, lo)) | blk.repeat_interleave(BLOCK, dim=-1)
    return blk, el


# ------------------------------------------------------------------------------------------------ zero-bar families: codes + exponents
def _gen(*key):
    return G._gen("fp8", *key)


def _exps(g, rows, nkb, lo, hi):
    return torch.randint(lo, hi + 1, (rows, nkb), generator=g, dtype=torch.int32)


ZERO_BAR = ("selector", "smallsum")
BARRED = ("randn", "offset", "heavy")


@functools.lru_cache(maxsize=6)
def zero_family(fam, M, N, K, wide=True):
    """-> dict Aq [M, K], Ae [M, K/32], Bq [N, K], Be [N, K/32] (uint8 codes, int32 exponents), bias [N], R [M, N] (fp32 integers).
    selector: row m of A holds ONE non-zero, (m % 3 + 1) * (+-1), at k = (5 m + 3) % K; B holds the integers ((3 n + 5 k) % 7) - 3; every 32-block
      of either operand has its own exponent, from -2..3 (wide) or 0..1: out[m, n] = a_m 2^eA B[n, k_m] 2^eB names the row, the K position, both
      scale bytes and the column.  wide=False keeps |out| <= 36 so that an integer bias and residual still leave a bf16 integer.
    smallsum: four non-zeros (+-1, +-2) per row of A, B in -3..3, exponents 0..1: |sum| <= 96, + bias + R (each |.| <= 8) <= 112.
    intsum (quantised output only): dense integers -3..3 on both sides, exponents 0..1: every partial sum is an integer below 2^24, exact in fp32
      and not in bf16.  Rows m % 64 == 7 of A hold only a 1 at k = 0 and rows m % 64 == 11 only a 15 at k = 1, and in every 32-block of B's rows
      column 0 holds -2..2 with one 4, column 1 holds -1..1 with one 1 (K-block 0 of those rows of A and of all of B has exponent 0): the output
      blocks of rows 7 have the maximum 4 = 2^2 exactly, those of rows 11 the maximum 15, which scales to 480, in (448, 512), and saturates."""
    g = _gen(fam, M, N, K, wide)
    nkb = K // BLOCK
    m, n, k = torch.arange(M), torch.arange(N), torch.arange(K)
    if fam == "selector":
        a = torch.zeros(M, K)
        a[m, (5 * m + 3) % K] = ((m % 3 + 1) * (1 - 2 * (m % 2))).float()
        b = (((3 * n[:, None] + 5 * k[None, :]) % 7) - 3).float()
        lo, hi = (-2, 3) if wide else (0, 1)
    elif fam == "smallsum":
        a = torch.zeros(M, K)
        cols = torch.rand(M, K, generator=g).argsort(1)[:, :4]
        a.scatter_(1, cols, (torch.randint(1, 3, (M, 4), generator=g) * (torch.randint(0, 2, (M, 4), generator=g) * 2 - 1)).float())
        b = torch.randint(-3, 4, (N, K), generator=g).float()
        lo, hi = 0, 1
    elif fam == "intsum":
        a = torch.randint(-3, 4, (M, K), generator=g).float()
        b = torch.randint(-3, 4, (N, K), generator=g).float()
        lo, hi = 0, 1
    else:
        raise ValueError(fam)
    ae, be = _exps(g, M, nkb, lo, hi), _exps(g, N, nkb, lo, hi)
    if fam == "intsum":
        p2, sat = m % 64 == 7, m % 64 == 11
        a[p2 | sat] = 0
        a[p2, 0] = 1.0
        a[sat, 1] = 15.0
        ae[p2 | sat, 0] = 0
        be[:, 0] = 0
        b[:, 0] = torch.randint(-2, 3, (N,), generator=g).float()
        b[:, 1] = torch.randint(-1, 2, (N,), generator=g).float()
        b[n % 32 == 5, 0] = 4.0
        b[n % 32 == 8, 1] = 1.0
    bias = torch.randint(-8, 9, (N,), generator=g).float()
    R = torch.randint(-8, 9, (M, N), generator=g).float()
    return dict(Aq=code_of(a), Ae=ae, Bq=code_of(b), Be=be, bias=bias, R=R)


def zero_product(d):
    """The exact product of a zero-bar family as a cheap fp32 host product: every decoded value is an integer times 2^-2 at least and every partial
    sum stays below 2^24 in units of the smallest one (zero_exact() asserts it), so fp32 holds each exactly in any order."""
    return decode(d["Aq"], d["Ae"]).to(F32) @ decode(d["Bq"], d["Be"]).to(F32).t()


def zero_exact(d, unit=2.0 ** -4):
    """The premise of zero_product and of the bar 0 on the device: sum_k |a_k b_k| < 2^24 units (then so is every partial sum in any order)."""
    sa = decode(d["Aq"], d["Ae"]).abs() @ decode(d["Bq"], d["Be"]).abs().t()
    return bool((sa / unit < 2.0 ** 24).all()) and bool(torch.equal(sa / unit, torch.round(sa / unit)))


# ------------------------------------------------------------------------------------------------ barred families: bf16 values for the quantiser
def barred_family(fam, M, N, K, seed=0):
    """-> dict A [M, K], W [N, K], bias [N], R [M, N]: fp32 tensors of bf16-exact values, quantised by the device.  randn: unit activations, weights
    of size K^-1/2.  offset: activations + 8 (long sums of one sign; the residual of the single-rounding check is refs64_gemm.cancel_R).  heavy: a
    few entries per row times 64, which dominate their blocks, next to blocks of size 1e-6 and all-zero blocks."""
    g = _gen(fam, M, N, K, seed)
    a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
    if fam == "offset":
        a = a + 8.0
    elif fam == "heavy":
        for t in (a, w):
            t[torch.rand(t.shape, generator=g) < 4.0 / K] *= 64.0
            blocks = t.view(t.shape[0], K // BLOCK, BLOCK)
            kind = torch.rand(blocks.shape[:2], generator=g)
            blocks[kind < 0.1] *= 1e-6
            blocks[kind > 0.9] = 0.0
    elif fam != "randn":
        raise ValueError(fam)
    return dict(A=G._bf(a), W=G._bf(w), bias=G._bf(torch.randn(N, generator=g)), R=G._bf(torch.randn(M, N, generator=g)))


# ------------------------------------------------------------------------------------------------ constructed quantiser blocks
def constructed_blocks(dtype):
    """[rows, 32] rows of `dtype` values that put the rule on its edges; every other element of a row is small against the named one.
    In order: amax exactly 2^k; amax = 448 2^e exactly; 464 2^e (the tie between 448 and the first value the format lacks: RNE would go to 512,
    the rule saturates); the largest bf16 below 2^(k+1) (scales to 510 and clamps); a tie to even in every e4m3 binade and in the subnormal
    range; -0.0; (fp32 only) one ulp to either side of a tie; a block of subnormals of the input format (e = -127, codes RNE(x 2^127))."""
    rows = []

    def row(vals, fill=0.0):
        r = torch.full((32,), fill, dtype=F64)
        r[:len(vals)] = torch.tensor(vals, dtype=F64)
        return r

    for k in (-20, -1, 0, 1, 7, 30):
        rows.append(row([2.0 ** k, -(2.0 ** k) * 0.75, 2.0 ** k * 0.3125]))
    for e in (-12, 0, 5):
        rows.append(row([448.0 * 2.0 ** e, -3.0 * 2.0 ** e]))
        rows.append(row([-464.0 * 2.0 ** e, 464.0 * 2.0 ** e, 17.0 * 2.0 ** e]))
    for k in (-3, 0, 9):
        rows.append(row([(2.0 - 2.0 ** -7) * 2.0 ** k, -(2.0 - 2.0 ** -7) * 2.0 ** k]))          # 1.1111111b 2^k: 510 after scaling
    # amax 256 (e = 0, the elements are their own scaled values): the midpoint between two neighbours in every binade 2^-6 .. 2^7, both parities of
    # the lower neighbour, and in the subnormal range (multiples of 2^-9 below 2^-6: midpoints at odd multiples of 2^-10)
    ties = [256.0]
    for b in range(-6, 8):
        for mant in (0, 1, 6):
            ties.append((1 + mant / 8.0 + 1 / 16.0) * 2.0 ** b * (-1 if mant == 1 else 1))
    rows.append(row(ties[:32]))
    rows.append(row([256.0] + ties[32:] + [m * 2.0 ** -10 for m in (1, 3, 5, 7, 9, 11, 13, 15)] + [-3 * 2.0 ** -10, 2.0 ** -11, -(2.0 ** -11) * 1.5]))
    rows.append(row([1.0, -0.0, 0.0, -0.0]))
    rows.append(row([-0.0] * 32))
    if dtype == F32:
        t = (1 + 1 / 16.0) * 2.0 ** 3          # 8.5: the tie between 8 and 9 under e = 0
        u = 2.0 ** -20                         # one fp32 ulp in [8, 16): a reader that drops the low 16 bits sees the tie itself
        rows.append(row([256.0, t + u, t - u, -(t + u), -(t - u), t, t + 1.0 + u, t + 1.0 - u]))
        sub = 2.0 ** -149
        rows.append(row([sub * v for v in (1, 2, 3, 5, 8, 9, 447, 448, 449, 1 << 20, (1 << 22) + 1, (1 << 23) - 1, -7, -(1 << 21))]))
    else:
        sub = 2.0 ** -133                       # bf16 subnormals: multiples of 2^-133 below 2^-126
        rows.append(row([sub * v for v in (1, 2, 3, 5, 8, 9, 17, 33, 65, 127, -7, -126)]))
    x = torch.stack(rows).to(dtype)
    assert torch.equal(x.double(), torch.stack(rows)), "a constructed value is not representable in the input format"
    return x


# ------------------------------------------------------------------------------------------------ case tables of tests/test_fp8_pin_gpu.py
# the entries of refs64_gemm.EPIS that avllm_gemm_f8 has a form for ("strided" is not a form of its own here: every operand of every call is a column
# slice of a wider buffer)
EPIS = tuple(e for e in G.EPIS if e.name in ("plain", "bias", "R", "bias_R", "R_inplace", "gelu", "quick_gelu", "silu"))
REF_M, REF_N, REF_K = (1, 17, 64, 65, 130, 257, 300), (8, 129, 200, 264, 1000), (128, 256, 384)
FAST_MN = ((2048, 2048), (2040, 2056), (16379, 256), (253, 16376))
FAST_K = (256, 384, 1024)
WALK_TILES = ((24, 22), (17, 16))          # 256 x 256 tiles, less 3 rows and 8 columns
WALK_K = (256, 384)
QOUT_MN = ((2048, 2048), (2040, 2048), (24 * 256 - 3, 22 * 256))
QOUT_ACTS = (G.ACT_NONE, G.ACT_GELU, G.ACT_QUICK_GELU, G.ACT_SILU)
QUANT_R, QUANT_K = (1, 15, 17, 63, 65, 255, 257, 300), (128, 384)
NORM_D, NORM_ROWS = (128, 768, 1152, 2176, 4096, 4224, 8192), (1, 63, 65, 257)
NORM_FAMILIES = ("randn", "heavy", "tiny", "const", "offset8")          # test_bytemovers_gpu.families(bf16)
NORM_EPS = 1e-5
# The largest share of (elements, blocks) of a norm case that its bar may leave undetermined, i.e. exempt from equality with the rule (or one element /
# block where a case is small); tests/test_fp8_refs_cpu.py asserts it for every case from the reference and the bar alone, so a bar that grew
# would fail there.  An element can move when a rounding boundary of its code lies within +-bar: with the e4m3 spacing |y| / 11.5 on average that is
# 23 bar / |y|, and over a unit-variance row E[1 / |y|] is about 8 (it stops growing 15 binades under the block maximum, where the spacing stops
# shrinking): 190 bar.  bars.fp32_bar is ONE number per tensor, so each family's figure follows from the size of its bar against its typical element:
#   randn, tiny : bar = 4 ulp of the largest element (5 sigma): 190 * 4 * 2^-23 * 5 / sigma = 5e-4 ... the 0.1 % of the rule.
#   offset8     : the same rows after normalisation, but x - mean at |x| = 8 costs 3 bits of x and the host's fp32 error, hence the bar, is 2 to 3
#                 times randn's: 0.3 %.
#   const       : RMSNorm gives y = w (c rstd) with c rstd = 1 - eps / 2 c^2: the bf16 w, which sits ON an e4m3 tie once in 16, moved by 4e-7 (c = 3.5)
#                 to 2e-5 (c = 0.5) of itself.  Where that is inside the bar (6e-7: the rows with |c| >= 3, at most 3 of the 7 row values) the tie is
#                 undetermined: 3/7 * 1/16 = 2.7 %, no block.  Under LayerNorm the result is the bias itself and EVERYTHING is determined: no exemption at
#                 all (norm_exact), so no cap applies.
#   heavy       : one entry of a row is 1e3 times the rest, so the bar, k * 4 ulp of THAT entry (k = 1 at fp32_bar's floor, up to 3 from the host's own
#                 error), is k * 2^-22 * 1e3 = k * 2.4e-4 of a typical element: 190 * 2.4e-4 = 4.6 % per unit of k, 15 % at k = 3.  A block maximum
#                 (3 sigma of 32) meets a power of two within the bar with probability 2 bar / (amax ln 2) = k * 2.3e-4, doubled for the blocks the
#                 outlier leaves in the subnormal range: 0.3 %.
MOVE_CAP = {"randn": (1e-3, 1e-3), "tiny": (1e-3, 1e-3), "offset8": (3e-3, 1e-3), "const": (3e-2, 1e-3), "heavy": (1.5e-1, 3e-3)}


def norm_exact(rms, fam):
    """const under LayerNorm: a constant row of multiples of 0.5 has an exact fp32 sum and mean, x - mean is exactly 0, and the result is the bf16 bias
    itself in the kernel as in float64: codes and exponents equal the rule's everywhere, ties included."""
    return fam == "const" and not rms


def norm_cases(rms, d):
    """(rows, family, want_y, want_rstd) of one norm and width: every row count with every family, the four want_y / want_rstd combinations
    rotating over them (each of the four occurs for every row count and every family)."""
    out = []
    for ri, rows in enumerate(NORM_ROWS):
        for fi, fam in enumerate(NORM_FAMILIES):
            c = (ri + fi) % 4
            out.append((rows, fam, bool(c & 1), bool(c & 2)))
    return out


def norm_ref(x, w, b, rms):
    """-> (float64 result, the same formula in fp32 on the host, float64 rstd [rows], fp32 rstd), from refs64; LayerNorm's rstd = rsqrt(var + eps)."""
    import refs64 as R64
    if rms:
        y, r = R64.rmsnorm_fwd(x, w, NORM_EPS)
        y32, r32 = R64.rmsnorm_fwd(x, w, NORM_EPS, dtype=F32)
        return y, y32, r, r32
    y32 = torch.nn.functional.layer_norm(x.float().cpu(), (x.shape[1],), w.float().cpu(), b.float().cpu(), NORM_EPS)
    x64, x32 = x.double().cpu(), x.float().cpu()
    return (R64.layernorm(x, w, b, NORM_EPS), y32, torch.rsqrt(x64.var(-1, unbiased=False) + NORM_EPS), torch.rsqrt(x32.var(-1, unbiased=False) + NORM_EPS))
