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
