"""Parity bars of the test-suite, stated ONCE (the tests import them; nothing restates a number).

fp32 mode (`precision="fp32"`: fp32 storage, exact-fp32 MFMA `v_mfma_f32_16x16x4_f32`) carries the north-star bar of
BASELINE.json: logits within 1e-3 of the reference, greedy tokens identical.  Observed differences are 1e-5 .. 5e-5 (summation
order only), so the bars below are the north-star's, not the observed ones.

bf16 mode (`precision="bf16"`: bf16 storage, fp32 accumulate / softmax / norm statistics / loss -- the arithmetic bench.py times)
cannot hold 1e-3 absolute through a transformer stack (SURVEY.md §7 "Hard parts"), so its bar is derived instead of observed:

  * bf16 keeps 8 significant bits: unit roundoff u = 2^-9 = 1.95e-3; a stored value carries a uniformly distributed relative
    rounding error of RMS u/sqrt(3) = 1.13e-3.
  * every tensor written to HBM is rounded once.  On the residual path of one decoder layer that is n ~ 8 roundings (normed input,
    q|k|v, attention output, o-projection+residual, normed input, gate|up, SwiGLU product, down-projection+residual); independent
    roundings add in quadrature, so after L layers the relative L2 error of the hidden state is about 1.13e-3 * sqrt(8 L):
    0.3 % for one layer, 0.45 % for the 2-layer golden model, 1.8 % for 32 layers.  The bf16 weights add one more rounding per
    product (same size, already in the sqrt).
  * the backward pass runs the same chain again on dY (another sqrt(2)) and the LoRA gradients are reductions over tokens of
    products of two rounded tensors: ~2x the forward figure.
  * bars = 4x these estimates at the depth the tests run (<= 2 layers), rounded up: a systematic error (a wrong mask, a dropped
    term, a mis-indexed tile) shows up as tens of percent and cannot hide under them.

The looser absolute logit bars (max / mean) are the same statement for O(1) logits and are kept for the golden-vector tests.
"""

# ---- fp32 mode: BASELINE.json north-star
F32_LOGITS_ABS = 1e-3            # max |logits - reference|
F32_LOSS_ABS = 1e-4
F32_GRAD_REL_MAX = 2e-4          # max |g - ref| <= this * max|ref| per LoRA tensor

# ---- bf16 mode (derived above)
BF16_LOGITS_REL_L2 = 2e-2        # ||logits - ref|| / ||ref|| over the whole tensor
BF16_LOGIT_MAX_ABS = 6e-2        # x max(1, max|ref|): tail of the same distribution over ~1e5 logits
BF16_LOGIT_MEAN_ABS = 1e-2
BF16_LOSS_ABS = 2e-2
BF16_GRAD_REL_L2 = 5e-2          # whole LoRA gradient, relative L2
BF16_GRAD_TENSOR_REL_L2 = 1e-1   # any single LoRA tensor (small tensors are noisier)
BF16_ENC_REL_L2 = 2e-2           # encoder outputs (Whisper hidden states, CLIP CLS), relative L2
# The encoders judged per output row (Whisper) / per frame (CLIP), tests/encoder_cases.py ratios(): BF16_ENC_REL_L2 and F32_LOGITS_ABS stand as
# they are -- the reference with a bf16 rounding at every store of the engine (refs64_encoders, rounded=True) stays within 0.20 .. 0.28 of
# BF16_ENC_REL_L2 on the worst row of every bf16 case with a block over five draws (tests/test_encoder_cases_cpu.py).
# Whisper with no block (layers = 0: the conv stem and the final LayerNorm alone) gets tight bars of its own:
#   bf16: four stores lie between the mel and the output (cols1, h1, x, out), u / sqrt(3) = 1.1e-3 relative each; the worst ROW of the
#   rounded restatement over five draws of three stems (320 / 768 / 1280 wide, 80 and 128 mels, with and without the low-variance plant)
#   reaches 3.42e-3; the bar is twice that.  The CPU file re-measures it (the worst row must lie in 0.25 .. 0.5 of the bar).
#   fp32: 100 x the distance of the fp32 host oracle from float64 on the same stems (1.2e-6 per row, printed by the CPU file); the K <= 3840
#   terms of conv2 summed in another order move a row by ~ sqrt(K) 2^-24 = 4e-6 in the mean.  A tenth of the bar the blocks are held to.
BF16_ENC_STEM_REL_L2 = 7e-3
F32_ENC_STEM_ABS = 1e-4


# ---- fp8 mode (BASELINE config 5: block-scaled e4m3 on the frozen projections of the forward pass, everything else as bf16).
# Against the oracle run WITH the same fake-quantisation (oracle/mxfp8.py): the products themselves are exact in fp32, so the difference is
# the bf16 path's difference plus quantisation DECISIONS that flip where the HIP path's bf16 activation and the oracle's fp32 activation
# straddle an e4m3 boundary (relative step 2^-3 .. 2^-4 on that element, averaged down by the K-length of the product: the test model's
# K = 128 .. 512 averages far less than the real widths' 1024 .. 14336; measured 6.9e-2 on its logits).  Bars = 3-5x bf16's.
# Against the UNquantised oracle the e4m3 noise itself shows (about 2^-4 / sqrt(3) per element and operand, ~3 % per product): the tests
# report it and only bound it loosely.
FP8_LOGITS_REL_L2 = 1e-1
FP8_LOSS_ABS = 6e-2
FP8_GRAD_REL_L2 = 1.5e-1
FP8_ENC_REL_L2 = 6e-2
# The fp8 encoders per frame (CLIP) / per block of 64 output rows (Whisper), against the reference that quantises each input where the case's
# launch forms do.  Yardstick: the two admissible readings of a quantiser's input, before or after its bf16 store (the fused and unfused
# forms of the same engine), differ per unit by at most 4.17e-2 over the eleven fp8 cases of tests/encoder_cases.py and three draws each
# (every Whisper case with a block lies at 3.7e-2 .. 4.2e-2, so no draw brings it under half of FP8_ENC_REL_L2); the bar is twice that,
# the factor the bf16 bars give their rounded restatement.  Re-measured by tests/test_encoder_cases_cpu.py.
FP8_ENC_UNIT_REL_L2 = 8.4e-2
FP8_VS_UNQUANTISED_REL_L2 = 2.5e-1
# Width does NOT shrink these bars (round 3, tests/test_fp8_gpu.py's config-5 family test at d = 1024 measured 6.4e-2 on the logits, the
# d = 128..512 model 6.9e-2).  Derivation: the HIP path quantises a bf16 activation, the oracle an fp32 one; they differ by delta ~ 4e-3
# (mean relative, a few bf16 roundings), so an element crosses an e4m3 rounding boundary with probability delta / step (step = mean relative
# e4m3 spacing, 2^-3 / 1.44 = 8.7e-2) and then moves by one step: relative L2 error of the quantised TENSOR = sqrt(delta / step) * step =
# sqrt(delta * step) = 1.9e-2, and a product with an independent operand passes that relative error on unchanged -- K-averaging reduces the
# absolute error of a sum and its magnitude alike.  About nine quantised activations lie on the path to the logits of a 2-layer LLM
# (x 3 in quadrature = 5.6e-2) plus the encoders' share: the 1e-1 / 6e-2 bars above are ~1.5x that, which is as tight as the rule allows.


# ---- bf16 at depth (tests/test_pin_bf16_gpu.py full-depth pin): the same derivation evaluated at the depth the bench runs instead of
# the <= 2 layers above.  Forward: u/sqrt(3) * sqrt(8 L) relative L2 on the hidden state (and the logits, a linear map of it); backward and
# LoRA gradients ~2x that (see above); the loss is a mean over ~30 scored tokens of log-probabilities whose logits carry that error.
BF16_DEPTH_FACTOR = 2.0          # bar = this x the estimate (the <= 2-layer bars above use 4x; at depth the estimate itself is larger: 1.8e-2 at L = 32,
                                 # where the first full-depth run measured 1.96e-2 on the logits and 3.0e-2 on the whole LoRA gradient)


def bf16_depth_rel_l2(layers, per_layer_roundings=8):
    return BF16_DEPTH_FACTOR * 1.13e-3 * (per_layer_roundings * layers) ** 0.5


def bf16_depth_grad_rel_l2(layers):
    return 2.0 * bf16_depth_rel_l2(layers)


def bf16_depth_loss_abs(layers):
    return BF16_LOSS_ABS * (layers / 2.0) ** 0.5


def fp8_depth_rel_l2(layers, per_layer_quantised=4):
    """fp8 against the unquantised arithmetic of the SAME model at depth: sqrt(delta * step) = 1.9e-2 relative L2 per quantised activation tensor
    (derivation above), four of them per decoder layer (the inputs of q|k|v, o, gate|up, down), independent -> in quadrature.  The encoders' share is
    left out: their outputs are pooled over frames before they reach the LLM.  1.9e-2 * sqrt(4 * 32) = 0.215 at L = 32 (measured: 0.164)."""
    return 1.9e-2 * (per_layer_quantised * layers) ** 0.5


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float(((a - b) ** 2).sum().sqrt() / (b ** 2).sum().sqrt().clamp_min(1e-30))


# ---- memory-bound kernels against float64 (tests/test_bytemovers_gpu.py, references in tests/refs64.py).  None of these bars comes from a
# kernel's output: each is the reference arithmetic's own fp32 error, the precision of the formats, or the derivation written here.
U32 = 2.0 ** -24                 # fp32 unit roundoff (half an ulp, relative); one ulp = 2 * U32
BF16_OUT_REL = 2.0 ** -8         # one round-to-nearest of a bf16 output is 2^-9 relative; doubled for ties moved by the fp32 error underneath
FP32_DENORM = 2.0 ** -126        # results below this may be flushed by the hardware exp2 / rcp: an absolute floor wherever they are used


def fp32_bar(ref64, cpu32):
    """fp32 kernels.  cpu32 = the same operation evaluated in fp32 on the HOST from the same inputs (torch's fp32 op where one exists, else the
    refs64 restatement run with dtype=float32); the measurement is made INSIDE the test, per case, so offset / heavy-tail families carry their
    own reachable accuracy (it degrades as eps * mu / sigma) and nothing is loosened by hand.  Bar (one number for the tensor) = 4 x max |cpu32 -
    ref64|, floored at 2 ulp of the output magnitude.  The factor 4 covers the different reduction order: the kernels add 64..256 lane partials
    serially-then-butterfly, torch adds pairwise."""
    e = float((cpu32.double() - ref64).abs().max())
    return max(4.0 * e, 2.0 * 2.0 * U32 * float(ref64.abs().max()))


def bf16_bar(ref64, fp32_bar_value):
    """bf16 outputs, elementwise: the fp32 bar of the arithmetic underneath plus 2^-8 |ref| for the final rounding."""
    return fp32_bar_value + BF16_OUT_REL * ref64.abs()


def expf_rel(arg, roundings=2):
    """Relative error of __expf(arg) = hardware exp2(arg * log2 e), elementwise on a float64 tensor of arguments.  The argument of exp2 is a rounded
    fp32 product (and log2 e a rounded constant; one more rounding when `arg` itself is a rounded product such as -1.702 x): `roundings` half-ulps
    of |arg| log2 e, i.e. an absolute error of roundings * |arg| log2(e) 2^-24 in the exponent, which exp2 turns into the relative error
    ln 2 * that = roundings * |arg| * 2^-24.  v_exp_f32 itself is specified to 1 ulp = 2^-23 relative.  This grows with |arg|, which is why torch's
    correctly rounded exp is not the yardstick for these kernels."""
    return roundings * arg.abs() * U32 + 2.0 * U32


def silu_bar(x, k=1.0):
    """|error| of x / (1 + __expf(-k x)) (SiLU: k = 1; quick-GELU: k = 1.702), elementwise, x float64.  With s = sigmoid(k x) and e = exp(-k x):
    dy/de * delta_e = |x| s (1 - s) * expf_rel; the add, the IEEE division and (k != 1) the product each round once: 3 half-ulps of |y|; results
    below the normal range may be flushed.  For -k x > ln(FLT_MAX) = 88.72 the exponential is +inf in fp32 and the result x / inf = -0 where the
    exact one is still a normal number of size <= |x| / FLT_MAX (2.6e-37): a property of the fp32 range, allowed for as that absolute term."""
    import torch
    s = torch.sigmoid(k * x)
    return x.abs() * s * (1 - s) * expf_rel(k * x, 2 if k == 1.0 else 3) + 3 * U32 * (x * s).abs() + FP32_DENORM + x.abs() / 3.4028e38


def swiglu_bwd_bar(dh, g, u):
    """[dg | du] of swiglu_bwd.  du = dh * silu(g): silu_bar * |dh| plus one rounding.  dg = dh u f with f = s (1 + g (1 - s)), s = 1 / (1 + e):
    delta_s = s (1 - s) expf_rel + 2 roundings of s (add, divide), and df/ds = 1 + g - 2 g s amplifies it (for g >> 1, 1 - s is a cancellation:
    its absolute error 2^-24 is multiplied by g); the four operations of f and the two products round once each, bounded on the magnitudes of
    the terms |s| + |g s (1 - s)|."""
    import torch
    s = torch.sigmoid(g)
    ds = s * (1 - s) * expf_rel(g) + 2 * U32 * s + FP32_DENORM          # (s itself goes denormal from g = -87.4 down, and may be flushed)
    f_terms = s + (g * s * (1 - s)).abs()
    bar_dg = (dh * u).abs() * ((1 + g - 2 * g * s).abs() * ds + 6 * U32 * f_terms) + FP32_DENORM
    bar_du = dh.abs() * silu_bar(g) + U32 * (dh * g * s).abs() + FP32_DENORM
    return torch.cat([bar_dg, bar_du], 1)


def ce_lse_expf_term(V):
    """What __expf adds to a row's log-sum-exp on top of fp32_bar: d lse = d(sum) / sum = sum_a e^a rel(a) / sum_a e^a with a = logit - max <= 0
    and rel(a) = expf_rel(a) = 2^-23 + 2 |a| 2^-24, i.e. 2^-23 + 2^-23 * E_p|a|, and E_p|a| = H(p) - log(sum) <= ln V for a softmax p.  The
    running-max rescale factors __expf(old max - new max) multiply terms that the same bound already covers (|a| e^-|a| <= 1/e)."""
    import math
    return 2.0 * U32 * (1.0 + math.log(max(V, 2)))


def rope_angle_bar(angle, ulps=4.0):
    """|error| of the fp32 angle the kernels form against HF's fp32 angle (both = position * inv_freq with inv_freq = 1 / theta^(2i/hd) in fp32),
    elementwise.  The two sides use different powf implementations (each within 1 ulp), a correctly rounded reciprocal and product each (half an
    ulp each): 4 ulp of the angle in all = 8 * 2^-24 |angle|.  At position 131 000 and inv_freq 1 that is 0.06 rad: a property of fp32 angles (the
    float64-angle distance the tests print is of the same size), not of a kernel.  cosf / sinf add 2 ulp of 1.  With the "llama3" rule both sides
    pass inv_freq through ten more fp32 operations (2 pi / inv, ctx / wavelen, - low, / (high - low), 1 - smooth, two products, / factor, +):
    half an ulp each and side = 10 ulp more: ulps = 14 for the frequencies the rule rescales or smooths (rope_llama3_ulps); the high frequencies
    it passes through untouched keep 4.  `ulps` is a number or a tensor that broadcasts against `angle`."""
    return 2.0 * ulps * U32 * angle.abs() + 4.0 * U32


def rope_llama3_ulps(hd, theta, scaling):
    """Per-frequency `ulps` [hd/2] for rope_angle_bar under HF's "llama3" rule: 4 where wavelen < ctx / high_freq_factor (inv_freq passes through
    torch.where untouched on both sides), 14 where it is divided by `factor` or smoothed.  Decided on the float64 wavelength with a 1e-5 margin
    towards 14, so a frequency an fp32 comparison could put on either side of the edge counts as touched."""
    import math
    import torch
    _, _, high, octx = scaling
    inv = 1.0 / (torch.tensor(theta, dtype=torch.float64) ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    untouched = 2 * math.pi / inv < (octx / high) * (1 - 1e-5)
    return torch.where(untouched, torch.tensor(4.0, dtype=torch.float64), torch.tensor(14.0, dtype=torch.float64))


def atomic_sum_term(n_adds, total):
    """What float atomics add to fp32_bar when n_adds non-negative partials are accumulated onto one fp32 word in ARRIVAL order (avllm_grad_sumsq):
    each add rounds the running total (<= total) by at most 2^-24 * total, the order is not fixed, so no tree-order factor covers it.  The roundings
    are independent and centred: standard deviation 2^-24 * total / sqrt(3) each, sqrt(n_adds) times that for the sum; the term is 4 sqrt(n_adds)
    2^-24 total = 6.9 standard deviations (7.6e-6 relative at 1024 adds; the worst case n_adds * 2^-24 would be 6e-5 and hide a dropped tail).
    The fixed-order form avllm_grad_sumsq_det is held to fp32_bar alone."""
    return 4.0 * n_adds ** 0.5 * U32 * abs(total)


# ---- attention against float64 (tests/test_attention_pin_gpu.py, references and the host emulation in tests/refs64_attention.py).  As above, no
# number here comes from a kernel's output.  A round-to-nearest to bf16 (8 significant bits: spacing 2^-7 in [1, 2)) moves x by at most half a
# spacing, 2^-8 relative for x just above a power of two and 2^-9 just below the next: the BOUND is 2^-8 = 2 x the 2^-9 the text above calls u
# (which is the size relative to the top of the binade).
BF16_U = 2.0 ** -8
# Rounding P to bf16 before the PV product.  The kernel forms o~ = sum_j p_j (1 + d_j) v_j / l with |d_j| <= u.
#   * l from the UNROUNDED p (attn_fwd_mfma): o~ - o = sum_j w_j d_j v_j, so |o~ - o| <= u sum_j w_j |v_j| (w = the float64 softmax).
#   * l from the ROUNDED p (attn_fwd_short): o~ = sum w (1 + d) v / sum w (1 + d) = o + sum w d (v - o) / (1 + sum w d), so
#     |o~ - o| <= u sum_j w_j |v_j - o| / (1 - u).
# Both are worst-case bounds (every d_j at +-u with the sign of its term), so the factor on the term is 1, times 1 / (1 - u) <= 1 + 2^-7 for the
# second form; the online softmax changes nothing (a tile's p is rounded relative to the running max of its time and later multiplied by fp32
# rescale factors, whose error the fp32 bar underneath carries).  A random-sign estimate would be sqrt(sum w^2) times smaller, which is what
# a correct kernel typically shows; a missing or extra key moves o by w_j |v_j - o|, the size of ONE term of the sum.
ATTN_P_ROUND = BF16_U * (1.0 + 2.0 ** -7)


def attn_out_bar(o64, w64_term, fp32_bar_value, rounded=True):
    """bf16 attention output, elementwise: 2^-8 |o| for the one final rounding (BF16_OUT_REL) + the P-rounding term above (w64_term = sum_j w_j |v_j - o|
    or sum_j w_j |v_j|, whichever the kernel's row sum calls for; None for the scalar kernels, which never round P) + the fp32 bar of the arithmetic
    underneath.  rounded=False (fp32 storage): the fp32 bar alone."""
    if not rounded:
        return fp32_bar_value + 0.0 * o64.abs()
    bar = fp32_bar_value + BF16_OUT_REL * o64.abs()
    return bar if w64_term is None else bar + ATTN_P_ROUND * w64_term


def attn_lse_bar(lse64, lse_cpu32, Tk):
    """LSE of either mode: the fp32 bar of the host's fp32 evaluation from the same inputs + what exp2 adds to a log-sum-exp over Tk terms
    (ce_lse_expf_term).  Nothing for bf16: the scores are fp32 sums of exact bf16 products and the row sum is an fp32 sum of fp32 exponentials."""
    return fp32_bar(lse64, lse_cpu32) + ce_lse_expf_term(Tk)


def attn_count_lse_bar(n):
    """count family (all scores 0): lse = ln n.  m = 0 and every p = 1 are exact and l = n is an exact integer, so what is left is log2 (v_log_f32,
    1 ulp), the product with the fp32 literal ln 2 (half an ulp + the literal's own 2^-25) or logf, and the sum with m: 4 ulp of ln n, and 2 ulp of 1
    absolute for n = 1, 2 where ln n is small.  One ulp is 2^-23 = 2 U32, so the factors below are 8 U32 and 4 U32.  ln(n + 1) - ln n = 3e-3 at
    n = 330 is three orders above this."""
    import torch
    return 8.0 * U32 * torch.log(n.double()) + 4.0 * U32


def attn_count_out_bar(o64, rounded=True):
    """count family: p = 1 exactly and V holds small integers, so every partial sum is exact in fp32 and o = (sum over the visible keys) * (1 / n):
    a reciprocal and a product, 2 ulp of |o| (= 4 U32 |o|: one ulp is 2 U32), + the final bf16 rounding; 1e-12 absolute is the float64 reference's
    own roundoff (a mean that is exactly 0 comes out as 1e-17 there)."""
    return (BF16_OUT_REL if rounded else 0.0) * o64.abs() + 4.0 * U32 * o64.abs() + 1e-12


def attn_decode_weight_term(Tk, v):
    """What the exp2 on the way to the softmax weights adds to a decode output that is not the count family's (there every p = 1 is exact): the
    weights' relative error sums to ce_lse_expf_term(Tk) at most (the same sum that moves the LSE), and a weight error e_j moves
    o = sum w_j v_j by e_j (v_j - o), bounded by the span of V, 2 max |v|."""
    return ce_lse_expf_term(Tk) * 2.0 * float(v.double().abs().max())


def attn_bwd_bar(ref64, emul):
    """bf16 backward, one number per tensor (dq, dk, dv): the fp32_bar rule with the host emulation of the documented arithmetic in the place of cpu32:
    4 x max |emul - ref64| measured inside the case (the 4 covers the different reduction order and a different draw of the same roundings: the
    kernel's stored O and LSE differ from the emulation's in their last bit, so its delta and P round elsewhere), floored at 2 ulp OF BF16 of the
    largest result (2 * 2^-8 max |ref|).  The tests add one more term to it, the fp32 bound underneath: attn_bwd_tensor_bar, below."""
    e = float((emul.double() - ref64).abs().max())
    return max(4.0 * e, 2.0 * BF16_OUT_REL * float(ref64.abs().max()))


def attn_bwd_tensor_bar(ref64, yard, under_elem, rounded=True, rotated=False):
    """The whole bar of one backward tensor (dq, dk or dv), or of the column slice of one kv head of it, as a number:
        rounded (bf16 storage): attn_bwd_bar(ref64, yard) with yard = the host emulation;
        fp32 storage:           fp32_bar(ref64, yard) with yard = the float64 restatement run in fp32 on the host;
      + max(under_elem), the largest element of the DERIVED fp32 bound of the backward's own arithmetic (attn_bwd_elem_bars with no bf16 rounding
        anywhere).  Neither yardstick's DISTANCE from the reference shows that error where the result is a cancellation (T = 1: dq = 0 exactly
        in float64 and in both yardsticks, while a kernel leaves the fp32 noise of dP - delta there, so 4 x 0 would be the bar) or where
        P = exp2(s - lse) is recomputed from a stored LSE (the restatement run in fp32 divides by the row sum instead and never forms a
        difference of two numbers of size 20).  In bf16 storage the term is about 1e3 below the rest; in fp32 storage it is of the size of
        fp32_bar itself, a few times it where the scores are large.
      rotated (the inverse rotary was applied to this tensor): an output a c + b s takes the errors of both halves of its pair,
        (|c| + |s|) max(under_elem) <= sqrt(2) max(under_elem); the rotation's own two products and one sum round at the size of the result
        (3 fp32 half-ulps, which the floor of either rule covers)."""
    rule = attn_bwd_bar if rounded else fp32_bar
    return rule(ref64, yard) + (2.0 ** 0.5 if rotated else 1.0) * float(under_elem.max())


def attn_bwd_rel_l2_bar(amp=0.0):
    """bf16 backward, relative L2 per tensor, beside attn_bwd_bar.  Independent roundings of RMS u / sqrt(3) = 1.13e-3 lie on the way to each result:
    the MFMA operand (P for dv, dS for dq and dk), the result itself, and the stored LSE's and scores' fp32 error (nothing at this scale): 2, plus
    for dq and dk the stored O inside delta = rowsum(dO * O), whose weight relative to dS is `amp` (refs64_attention.delta_amplification: about 1
    for centred V, mu / sigma for an offset V, large where dS is a cancellation): 1.13e-3 sqrt(2 + amp^2), and 4 x that as everywhere in this file."""
    return 4.0 * 1.13e-3 * (2.0 + amp * amp) ** 0.5


def attn_bwd_elem_bars(q, k, v, dout, B, T, H, Hkv, hd, causal, scale, rounded=True, p_rounded=True):
    """Elementwise bars (bar_dq, bar_dk, bar_dv) of the backward from its float64 quantities, used where the result is structured and a per-tensor
    maximum would hide a row (the count family).  With u = 2^-8 (0 where the kernel does not round that operand) and r_p the fp32 error of
    P = exp2(s sl - lse log2e), 8 * 2^-24 (1 + |s scale| + |lse|) relative (two products rounded at the size of their result, the stored LSE's own
    few ulp, v_exp_f32's 1 ulp, doubled):
        |d P_ij|  <= w_ij (u + r_p)                              dv_j : sum_i |d P_ij| |dO_i|
        |d delta_i| <= u sum_d |dO_id o_id|                      (the stored O is rounded once)
        |d dS_ij| <= |dS_ij| (u + r_p) + w_ij scale (|d delta_i| + 8 * 2^-24 sum_d |dO_id v_jd|)
        dq_i : sum_j |d dS_ij| |k_j|,    dk_j : sum_i |d dS_ij| |q_i|    (summed over the query heads of a group)
    + 2^-8 |result| for the stored rounding + 2 fp32 ulp of the sum of magnitudes for the accumulation."""
    import torch
    import refs64_attention as A
    hm = A.head_map(H, Hkv)
    q4, k4, v4 = A._heads(q, B, T, H, hd, A.F64), A._heads(k, B, T, Hkv, hd, A.F64)[:, hm], A._heads(v, B, T, Hkv, hd, A.F64)[:, hm]
    do4 = A._heads(dout, B, T, H, hd, A.F64)
    vis = A.visible(T, T, causal)
    o4, lse, w = A._fwd_core(q4, k4, v4, vis, scale)
    s = (torch.einsum("bhid,bhjd->bhij", q4, k4) * scale).abs()
    u = BF16_U if p_rounded else 0.0
    uo = BF16_U if rounded else 0.0
    r_p = 8.0 * U32 * (1.0 + s + lse.abs()[..., None])
    dp = torch.einsum("bhid,bhjd->bhij", do4, v4)
    delta = (do4 * o4).sum(-1, keepdim=True)
    ds = w * (dp - delta) * scale
    e_p = w * (u + r_p)
    e_delta = uo * (do4 * o4).abs().sum(-1, keepdim=True)
    e_dp = 8.0 * U32 * torch.einsum("bhid,bhjd->bhij", do4.abs(), v4.abs())
    e_ds = ds.abs() * (u + r_p) + w * scale * (e_delta + e_dp)
    acc = 4.0 * U32
    dq4, dk4, dv4 = A._bwd_core(q4, k4, v4, do4, vis, scale)
    bq = torch.einsum("bhij,bhjd->bhid", e_ds + acc * ds.abs(), k4.abs())
    bk = A._group_sum(torch.einsum("bhij,bhid->bhjd", e_ds + acc * ds.abs(), q4.abs()), Hkv)
    bv = A._group_sum(torch.einsum("bhij,bhid->bhjd", e_p + acc * w, do4.abs()), Hkv)
    out = uo and BF16_OUT_REL
    bq = bq + out * dq4.abs()
    bk = bk + out * A._group_sum(dk4, Hkv).abs()
    bv = bv + out * A._group_sum(dv4, Hkv).abs()
    return A._rows(bq) + FP32_DENORM, A._rows(bk) + FP32_DENORM, A._rows(bv) + FP32_DENORM


# ---- GEMM against float64 (tests/test_gemm_pin_gpu.py, references, families and the host emulation in tests/refs64_gemm.py).  No number here comes
# from a kernel's output.  The exact and locate families carry the bar 0: their operands are small integers, every product and partial sum is
# an integer the fp32 accumulator holds exactly, and the result is representable in the output format, so ANY difference is an error.
# For the other families the accumulator's error is bounded ELEMENTWISE on sum_abs = sum_k |a_k| |b_k| (bf16 x bf16 products are exact in fp32, so
# only the additions round):
#   f32   : v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain: (K + K2) roundings, each at most 2^-24 of the running sum <= sum_abs.
#   mfma  : the bf16 MFMA's internal summation of its 32 products is not documented; any order of n - 1 round-to-nearest additions stays under
#           n 2^-24 sum_abs.  GEMM_MFMA_ALLOW = 2 is for the one thing that bound assumes and the hardware may not do: round-to-NEAREST inside the
#           instruction.  An adder that truncates the aligned addends loses up to one ulp per addition instead of half of one, i.e. 2 x.
#   split8: SMALLM and SKINNY64 add the 8 waves' partials in LDS order: 8 more roundings at the size of sum_abs.
#   tn    : gemm_tn adds up to 32 chunk partials with float atomics in arrival order onto the prior output: atomic_sum_term.
#   (The block-scaled fp8 MFMA, v_mfma_scale_f32_16x16x128_f8f6f4, does NOT stay under this bound: inside each group of 8 products it cuts below
#   2^-13 of the group's largest.  Measured and derived at the end of this file, "block-scaled fp8 against float64": fp8_gemm_bar adds
#   refs64_fp8.mfma_group_loss to the accumulator bar; tools/fp8_mfma_probe.py repeats the measurement.)
GEMM_MFMA_ALLOW = 2.0


def gemm_acc_bar(sum_abs, kk, kind):
    """|fp32 accumulator - exact sum|, elementwise; kk = the reduction length (K + K2, or the rows M of gemm_tn)."""
    if kind == "f32":
        return kk * U32 * sum_abs
    bar = GEMM_MFMA_ALLOW * kk * U32 * sum_abs
    if kind == "split8":
        bar = bar + 8.0 * U32 * sum_abs
    return bar


def gelu_fast_bar(z):
    """|error| of act_apply_fast's GELU = 0.5 z (1 + erf_AS(z / sqrt 2)), elementwise, z float64.  With x = |z| / sqrt 2, t = rcp(1 + 0.3275911 x),
    S(t) = sum |a_i| t^i and E = exp(-x^2): the Abramowitz-Stegun 7.1.26 formula is within 1.5e-7 of erf (common.h's comment); each of the five Horner
    stages multiplies by t (relative error <= 4 half-ulps: a product, a sum, rcp's 1 ulp) and rounds twice: 30 half-ulps of S(t); exp2's argument is
    two rounded products (2 x^2 half-ulps relative on E) and v_exp_f32 is 1 ulp (2 more); the subtraction from 1 rounds once.  The erf error is
    multiplied by 0.5 |z|; the sum 1 + erf and the two products round once each at the size of the result."""
    import math
    import torch
    x = z.abs() / math.sqrt(2.0)
    t = 1.0 / (1.0 + 0.3275911 * x)
    S = t * (0.254829592 + t * (0.284496736 + t * (1.421413741 + t * (1.453152027 + t * 1.061405429))))
    E = torch.exp(-x * x)
    e_erf = 1.5e-7 + U32 * (S * E * (32.0 + 2.0 * x * x) + 1.0)
    y = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    return 0.5 * z.abs() * e_erf + 3.0 * U32 * y.abs() + FP32_DENORM


def gelu_libm_bar(z):
    """act_apply's GELU: libm erff (a few ulp: 4 ulp of |erf| <= 1 taken), the product z / sqrt 2 (half an ulp of the argument, through
    erf' <= 2 / sqrt pi), then the sum and two products as above."""
    import math
    import torch
    y = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    return 0.5 * z.abs() * (8.0 * U32 + U32 * z.abs() * torch.exp(-0.5 * z * z)) + 3.0 * U32 * y.abs() + FP32_DENORM


def gemm_act_bar(z, act, libm=None):
    """The activation's own error at the float64 pre-activation z.  libm: True = act_apply (f32, 4-column and small-M epilogues), False =
    act_apply_fast (x * rcp(1 + exp2(c x)): silu_bar with one more ulp for v_rcp_f32 in place of the IEEE division), None = whichever is larger (a
    kernel that takes either epilogue by alignment)."""
    import torch
    if act == 0:
        return torch.zeros_like(z)
    if act == 1:
        lib, fast = gelu_libm_bar(z), gelu_fast_bar(z)
    else:
        k = 1.702 if act == 2 else 1.0
        lib = silu_bar(z, k)
        fast = lib + 2.0 * U32 * (z * torch.sigmoid(k * z)).abs() + FP32_DENORM * z.abs()      # v_rcp_f32 flushes a result below 2^-126 (1 + e > 2^126, k z < -87.3) that the
                                                                                                # product with z would have brought back into the normal range; the division does not
    return lib if libm is True else fast if libm is False else torch.maximum(lib, fast)


def gemm_bar(ref, kk, kind, act=0, alpha=1.0, out_bf16=True, libm=None):
    """Elementwise bar of one avllm_gemm call from its float64 reference `ref` (refs64_gemm.Ref: out, sum_abs, z, acc, mask).  The accumulator bar is
    carried through alpha (one rounded product, one rounded sum with the bias), through |act'(z)| plus the activation's own error, through the mask's
    scale (one rounded product), the residual sum rounds once at the size of the result, and a bf16 store adds BF16_OUT_REL |ref| -- ONCE: this is
    the single-rounding statement the offset family (R = -z + noise) holds a kernel to."""
    import refs64_gemm as G
    e = abs(alpha) * gemm_acc_bar(ref.sum_abs, kk, kind) + U32 * ((alpha * ref.acc).abs() + ref.z.abs())
    y = ref.z
    if act:
        y = G.act64(ref.z, act)
        e = G.dact64(ref.z, act).abs() * e + gemm_act_bar(ref.z, act, libm)
    if ref.mask is not None:
        e = ref.mask * e + U32 * (y * ref.mask).abs()
    e = e + U32 * ref.out.abs() + FP32_DENORM
    return e + BF16_OUT_REL * ref.out.abs() if out_bf16 else e


def gemm_tn_bar(ref, M, alpha, out0, mfma):
    """gemm_tn / gemm_tn_drop, fp32 output: the chunk partials (MFMA: any-order bound with the allowance; scalar kernel: an M-long fmaf chain), the
    product with alpha, and <= 32 float atomics in arrival order onto the prior output, whose running total stays under |out0| + |alpha| sum_abs."""
    total = out0.abs() + abs(alpha) * ref.sum_abs
    return abs(alpha) * gemm_acc_bar(ref.sum_abs, M, "mfma" if mfma else "f32") + U32 * (alpha * ref.acc).abs() + atomic_sum_term(32, total) + FP32_DENORM


# ---- LoRA adapter kernels against float64 (tests/test_lora_pin_gpu.py; references, families and the host emulation in tests/refs64_lora.py).  No
# number here comes from a kernel's output; the exact and locate families carry the bar 0 (integer operands, every partial sum an integer the fp32
# accumulator holds, the result representable in the output format).
#   rank3    : the arithmetic of SKINNY64: 8 waves split K, MFMA partials added in LDS in wave order, times alpha, one bf16 rounding: gemm_bar's
#              "split8".  The fused mask is part of the OPERAND (scaled survivors re-rounded to bf16, in the reference too), so it adds no term.
#   tn_multi : the arithmetic of gemm_tn's MFMA kernel: chunk partials over 64-row slabs, times alpha, at most 32 float atomics (the chunk cap of
#              tn_chunks) in arrival order onto the prior output: gemm_tn_bar.
#   dx_masked: per adapter ONE 32-slot MFMA from a zero accumulator (any-order bound with the allowance, on S_j = sum |t| |a|), one rounded product
#              with the mask's scale, then nj + 1 fp32 additions (the nj masked products onto a zero accumulator, then R) whose running total stays
#              under sum_j |scale p_j| over the adapters the mask KEEPS + |R| (a dropped product adds an exact 0), the denormal floor, and
#              BF16_OUT_REL |ref| ONCE: the header's "rounded once", which the offset family (R = -sum + noise) holds the kernel to.
def lora_rank3_bar(ref, K, alpha):
    return gemm_bar(ref, K, "split8", alpha=alpha, out_bf16=True)


def lora_tn_multi_bar(ref, M, alpha, out0):
    return gemm_tn_bar(ref, M, alpha, out0, mfma=True)


def lora_dx_bar(ref):
    """ref: refs64_lora.RefDx (out, prods, sum_abs, keeps, scale, R) -> elementwise bar, float64 [M, N]."""
    import torch
    e, total = torch.zeros_like(ref.out), ref.R.abs().clone()
    for pj, sj, k in zip(ref.prods, ref.sum_abs, ref.keeps):
        kept = k.to(ref.out.dtype)
        e = e + kept * (ref.scale * GEMM_MFMA_ALLOW * 32.0 * U32 * sj + U32 * (ref.scale * pj).abs())
        total = total + kept * (ref.scale * pj).abs()
    return e + (len(ref.prods) + 1) * U32 * total + FP32_DENORM + BF16_OUT_REL * ref.out.abs()


# ---- the fused token-step projection against float64 (tests/test_decode_pin_gpu.py; restatement, host emulation and cases in tests/refs64_decode.py).
# No number here comes from a kernel's output.  The chain, in the kernel's order, each term elementwise on the float64 quantities of
# refs64_decode.dec_proj64 (`ref`):
#   accumulator: gemm_acc_bar(sum_abs, K, "split8") -- bf16 x bf16 products are exact, the MFMA's internal order is not documented (any-order bound
#                with the allowance), the 8 wave partials meet in LDS order.  The fold xg = bf16(x g) is an exact fp32 product rounded once, in
#                the reference too, so it adds nothing.  exact / locate: 0 (every partial sum is held by fp32; the tests check that premise).
#   norm:        s = acc * rstd.  t = sum x^2 is K positive fp32 additions of exact squares (a lane's chain, 2 butterfly additions over the
#                lane columns, 8 wave partials): any order of n additions of positive terms stays under n 2^-24 relative, n = K + 10; the division
#                by K and the sum with eps round once each; the power -1/2 halves the relative error: (K + 12) / 2 half-ulps.  rsqrtf: the HIP
#                programming guide's table of device math functions lists rsqrtf with a maximum error of 1 ulp (it is v_rsq_f32); DEC_RSQRT_ULP = 2
#                is taken, the second ulp for the denormal-input scaling sequence around the instruction, = 4 half-ulps.  Then the product rounds once.
#   bias:        one rounded sum.
#   adapters:    u = a 16-term fmaf chain: 16 2^-24 sum |lt| |lb|, times |scale|; the product scale * u and the sum round once each (two roundings;
#                a contracted fma rounds once and is covered).
#   residual:    one rounded sum.
#   SwiGLU:      silu(g) * up with the errors e_g, e_up of both columns: |up| (|silu'(g)| e_g + silu_bar(g)) + |silu(g)| e_up + the cross term, the
#                second-order term of silu (|silu''| <= 1/2) and the rounded product.  silu_bar carries __expf (expf_rel), the sum and the division.
#   rotation:    o = z c -+ z' s with the fp32 table the reference reads too: |c| e_z + |s| e_z' + the two rounded products and the rounded sum.
#                The compiler may contract one product into an fma, which rounds less: the bound of the uncontracted form covers both.
#   output:      BF16_OUT_REL |out| ONCE for a bf16 output (the single-rounding statement the offset family, R = -z + noise, holds the kernel to),
#                and FP32_DENORM.
DEC_RSQRT_ULP = 2.0


def dec_rstd_rel(K):
    """Relative error of the kernel's fp32 rstd = rsqrtf(sum x^2 / K + eps) (derivation above)."""
    return (0.5 * (K + 12) + 2.0 * DEC_RSQRT_ULP) * U32


def dec_proj_bar(ref, exact=False):
    """Elementwise bar [M, N out] of one avllm_dec_proj launch from refs64_decode.dec_proj64's namespace.  exact: the accumulator (and the adapter
    chain, whose operands are then small integers too) carries 0."""
    import torch
    K = ref.K
    e = torch.zeros_like(ref.acc) if exact else gemm_acc_bar(ref.sum_abs, K, "split8")
    if ref.rstd is not None:
        e = ref.rstd * e + ref.y.abs() * dec_rstd_rel(K) + U32 * ref.y.abs()
    if ref.bias:
        e = e + U32 * ref.zb.abs()
    if ref.u is not None:
        chain = 0.0 if exact else 16.0 * U32 * ref.u_abs
        e = e + abs(ref.scale) * chain + U32 * ((ref.scale * ref.u).abs() + ref.z.abs())
    if ref.mode == 0:
        if ref.R is not None:
            e = e + U32 * ref.out.abs()
    elif ref.mode == 1:
        F = ref.F
        g, up, eg, eu = ref.z[:, :F], ref.z[:, F:], e[:, :F], e[:, F:]
        s = torch.sigmoid(g)
        d_silu = (s + g * s * (1 - s)).abs()
        e_silu = d_silu * eg + 0.5 * eg * eg + silu_bar(g)
        e = up.abs() * e_silu + (g * s).abs() * eu + e_silu * eu + U32 * ref.out.abs()
    else:
        c, sn, p = ref.cosv[None, :], ref.sinv[None, :], ref.partner
        rotary = (sn != 0) | (c != 1)
        zp = ref.z[:, p]
        e = torch.where(rotary, c.abs() * e + sn.abs() * e[:, p] + U32 * ((ref.z * c).abs() + (zp * sn).abs() + ref.out.abs()), e)
    e = e + FP32_DENORM
    return e if ref.out_f32 else e + BF16_OUT_REL * ref.out.abs()


# ---- token selection against float64 (tests/test_select_pin_gpu.py; restatements, host emulations and families in tests/refs64_select.py).  No
# number here comes from a kernel's output.  The kernels (sample.hip, beam.hip, token_score.hip, the log-softmax stage of logits_process.hip) form
# y = x / t (one IEEE division), d = y - m against the row maximum, e = expf(d), a sum of the e, its logarithm and one or two more sums.  The exact
# family of beam_topk(logprobs=True) carries the bar 0: its log-probabilities and beam scores are multiples of 2^-3 in [-16, 0], every sum is a
# multiple of 2^-3 below 32 and exact in fp32, so the whole order, ties included, is determined.
def _t64(a):
    import torch
    return torch.as_tensor(a).double()


def select_logprob_bar(ref64, cpu32, V, sizes=()):
    """A log-probability (row_scores, the score of a sample_rows draw, a row of the log-softmax stage) or a beam_topk score, one number per tensor:
    fp32_bar of the host's fp32 evaluation of the same formula from the same inputs (the different order of the V-term sum, the logarithm)
    + ce_lse_expf_term(V), what the exponentials add to the log of their sum (the bound holds for any libm within expf_rel, not only __expf)
    + one rounding (2^-24 relative) for each of the division, the subtraction from the maximum and the final sums, at the size of their results:
    `sizes` holds the float64 magnitudes |y|, |y - m|, |y - m - log s| and, for beam_topk, |beam score + log p| (tensors or numbers; the
    largest entry of each counts).  Entries of -inf are compared exactly by the tests and must not be passed in."""
    import torch
    extra = sum(float(_t64(s).abs().max()) for s in sizes)
    return fp32_bar(_t64(ref64), torch.as_tensor(cpu32)) + ce_lse_expf_term(V) + U32 * extra


def select_entropy_bar(y64, ent64, ent_cpu32):
    """row_scores' entropy H = log s - t / s with d_i = y_i - m <= 0, e_i = expf(d_i), s = sum e_i, t = sum e_i d_i, one number per row set.  With
    r_i = expf_rel(d_i) the relative error of e_i:  |ds| <= sum e_i r_i,  |dt| <= sum e_i |d_i| r_i, and
        |dH| <= |ds| / s + |dt| / s + |t| |ds| / s^2 = sum_i p_i r_i (1 + |d_i| + |t| / s),   p = e / s,
    elementwise over the row and summed (the rescale factors expf(old max - new max) of the online form multiply partial sums that the same bound
    covers, as in ce_lse_expf_term), + fp32_bar of the host's fp32 evaluation for the sums' order, the logarithm and the division.  y64 [rows, V]:
    the scaled rows in float64, -inf where banned."""
    import torch
    y = _t64(y64)
    m = y.max(-1, keepdim=True).values
    d = torch.where(torch.isinf(y), torch.zeros_like(y), y - m)
    e = torch.where(torch.isinf(y), torch.zeros_like(y), torch.exp(d))
    s = e.sum(-1, keepdim=True)
    t = (e * d).sum(-1, keepdim=True)
    term = ((e / s) * expf_rel(d) * (1.0 + d.abs() + t.abs() / s)).sum(-1)
    return float(term.max()) + fp32_bar(_t64(ent64), torch.as_tensor(ent_cpu32))


def draw_cdf_tol(probs, d, n_kept, W):
    """|a sample_rows CDF prefix - the float64 one|, both relative to their totals.  The kernel's prefix is sum_{i < j} w_i / sum_i w_i with
    w_i = floor(expf(d_i) 2^40): a relative error expf_rel(d_i) on each term moves a ratio of two such sums by at most 2 sum_i p_i expf_rel(d_i)
    (numerator and denominator, each at most sum_i p_i r_i); the truncation loses under 2^-40 per kept token of a total W = sum exp(d_i) (>= 1:
    the maximum is kept); the target floor(W u) and u's own 24-bit grid are worth 2^-23 together.  probs, d: the float64 probabilities and
    y_i - max of the kept tokens.  The same number is the delta of refs64_select.kept_band: top-p compares such a prefix with top_p."""
    p, dd = _t64(probs), _t64(d)
    return float(2.0 * (p * expf_rel(dd)).sum()) + n_kept * 2.0 ** -40 / W + 2.0 ** -23


# ---- block-scaled fp8 against float64 (tests/test_fp8_pin_gpu.py; references, families and the quantised-output rules in tests/refs64_fp8.py).  No
# number here comes from a kernel's output.
#   operands : an MX operand is exact by construction: decode(code) 2^e.  The reference is formed from the codes and scale bytes the kernel READS
#              (hand-built for the zero-bar families, read back from avllm_mx_quantize for the others), so quantisation error is not part of any bar.
#   products : e4m3 x e4m3 has 8 significant bits and the two block scales only move the exponent: every product is exact in fp32.  Only the
#              additions round, so gemm_bar(ref, K, "mfma", act, out_bf16=..., libm=False) applies as written: the any-order bound K 2^-24 sum_abs
#              with GEMM_MFMA_ALLOW for an adder that truncates, act_apply_fast's error, one bf16 rounding.  v_mfma_scale_f32_16x16x128_f8f6f4 sums
#              128 products per instruction and its internal order and alignment width are not documented; the tests print the worst ratio to this
#              bar per kernel, family and epilogue (profiles/r16_fp8_pin_ratios.txt holds the table).
#   zero bar : selector, smallsum (bf16 output) and intsum (quantised output): integer operands times small powers of two, every partial sum an
#              integer below 2^24 in units of the smallest product, the result representable in the output format (tests/test_fp8_refs_cpu.py checks
#              these premises on the host).  Any difference is an error; for intsum codes and the WHOLE scale image equal the rule's, bit for bit.
#   quantised output (the fast kernel's epilogue, avllm_norm_mxq): the kernel quantises an fp32 value v with |v - ref| <= bar, so
#              - its block exponent is one the rule gives for SOME maximum in [max(|ref| - bar), max(|ref| + bar)] (refs64_fp8.admissible_exps), and
#              - under that exponent e: |decode(code) 2^e - ref| <= step / 2 * 2^e + bar, step = the e4m3 spacing at (|ref| + bar) 2^-e (2^-9 in the
#                subnormal range), and where that magnitude passes 448 the element may be the clamp's 448 (refs64_fp8.quant_errors),
#              for every block and element, no share exempted.  bar = gemm_bar(..., out_bf16=False), or for the norms fp32_bar(ref64, cpu32).
#              Where neither the exponent nor the code can differ within the bar (refs64_fp8.can_move, from the reference alone) both EQUAL the rule's.
#   the instruction: v_mfma_scale_f32_16x16x128_f8f6f4 does NOT stay under the any-order bound, GEMM_MFMA_ALLOW included: the heavy family (a few
#              entries 64 times the rest) missed it by up to 8 x under BOTH kernels on the same elements while every zero-bar case held.  Measured
#              with constructed single-K-step cases (tools/fp8_mfma_probe.py -> profiles/r16_fp8_mfma_probe.txt: +P and -P cancel, small products v 2^-j of known sum beside):
#              - in each group of 8 consecutive k the products are aligned to the group's largest exponent sum E_g = max ex(a_k) + ex(b_k)
#                (ex = exponent field - 7; a subnormal counts as -6, a zero operand sets nothing) and CUT TOWARDS ZERO below 2^(E_g - 13): beside
#                P = 2^16 a product 2^3 survives and 2^2 does not, 1.875 2^5 comes out as 1.75 2^5, either sign alike; beside P = 2^-9 * 2^8 (a
#                subnormal operand) the cut sits at 2^(2 - 13), not 2^(-1 - 13);
#              - across groups nothing of the kind happens.  The neighbouring group of 8 (k = 8..15 beside P at k = 0) meets P's group at 2^-24 of P,
#                cut downwards (floor), exactly as the accumulator input is; farther away (another 16, another block) small products are kept down
#                to 2^-27 of P, rounded to nearest, and vanish only 28 binades below.  That is at most one unit of 2^-24 of the largest product per
#                group of 8 and per accumulator input, K / 8 + K / 128 units in all: inside K 2^-24 sum_abs with the allowance 2.
#              Derivation of the extra term: a product cut towards zero to a multiple of c = 2^(E_g - 13) (times the group's two block scales) loses
#              exactly |a_k b_k| mod c: nothing where its exponent sum is within 7 of E_g (an e4m3 product has 8 significant bits), less than c and
#              at most itself elsewhere.  The sum over k of these losses, from the CODES the kernel read (refs64_fp8.mfma_group_loss), bounds the
#              error; the products' signs may cancel part of it.  It is 0 for the zero-bar families (asserted on the host), below the any-order
#              term for operands of one scale (randn, offset) and ten to forty times it for heavy.  It enters gemm_bar as part of the accumulator bar.
def fp8_gemm_bar(ref, K, act=0, out_bf16=True, loss=None):
    """loss: refs64_fp8.mfma_group_loss of the operands (same rows as ref), or None where it is known to be 0."""
    if loss is not None:
        ref = ref._replace(sum_abs=ref.sum_abs + loss / (GEMM_MFMA_ALLOW * K * U32))          # gemm_acc_bar(sum_abs) + loss, through gemm_bar's chain
    return gemm_bar(ref, K, "mfma", act, 1.0, out_bf16, libm=False)


def ln_rstd_bar(x64):
    """fp32 rstd = rsqrt(var + eps) of LayerNorm rows x64 [rows, d] (avllm_norm_mxq's optional output), relative, per row.  A computed mean off by
    delta moves mean((x - m)^2) by exactly delta^2, and delta <= d 2^-24 mean|x| for any order of the sum; the d squares of differences rounded once
    each (3 half-ulps relative per term) add up in any order within (d + 3) 2^-24; the division and the sum with eps round once each; the power
    -1/2 halves it; rsqrtf is within DEC_RSQRT_ULP ulp."""
    d = x64.shape[-1]
    var = x64.var(-1, unbiased=False)
    delta = d * U32 * x64.abs().mean(-1)
    return 0.5 * ((d + 5) * U32 + delta * delta / var.clamp_min(1e-300)) + 2.0 * DEC_RSQRT_ULP * U32
