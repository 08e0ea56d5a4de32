"""Bars of avllm_qk_norm_rope / avllm_qk_norm_bwd against float64 (tests/refs64_qk_norm.py), built from the constants and rules of tests/bars.py.
No number here comes from a kernel's output.

Forward, elementwise, in the kernel's order:
  rstd      rsqrtf(sum x^2 / hd + eps): the derivation of bars.dec_rstd_rel with K = hd (hd positive additions in any order -- a lane's chain and
            the butterfly over the head's lanes -- the exact division by a power of two, the sum with eps, the power -1/2, rsqrtf's ulps).  The
            squares of bf16 inputs are exact in fp32; the squares of fp32 inputs round once each: U32 more on the sum, half of it on rstd.
  y         (x * rstd) * w: the rstd term and two rounded products.
  rotation  o = y c -+ y' s from the fp32 table the reference reads too: bars.dec_proj_bar's rotation term, |c| e_y + |s| e_y' + the two rounded
            products and the rounded sum (an fma contraction rounds less).
  output    BF16_OUT_REL |o| ONCE for a bf16 buffer, and FP32_DENORM.
  The saved rstd is held to the rstd term alone; the saved pre-norm copy, the v slice and the padding to equality of bytes.

Backward: rstd is an input of the kernel and of the restatement alike, so the arithmetic is hd products and additions and a handful of roundings
per element, with no transcendental: the fp32_bar rule against the restatement evaluated in fp32 on the host, measured inside each case, plus
BF16_OUT_REL |dx| for a bf16 buffer.  The radial family (g parallel to xhat: the exact result is 0 up to eps) would make that 4 x 0, so its bar
is the absolute bound of the cancellation instead: mean(g xhat) is hd rounded products and hd additions, (hd + 1) U32 max|g| max|xhat| at
most; its product with xhat, the difference and the product with rstd round once each at the size of |g| max(1, xhat^2):
(hd + 4) U32 max|g| max(1, max xhat^2) rstd per head."""
import torch

from bars import BF16_OUT_REL, FP32_DENORM, U32, dec_rstd_rel, fp32_bar


def rstd_rel(hd, fp32_in):
    return dec_rstd_rel(hd) + (0.5 * U32 if fp32_in else 0.0)


def rstd_bar(ref, fp32_in):
    return ref.rstd * rstd_rel(ref.hd, fp32_in)


def fwd_bar(ref, rounded):
    """Elementwise [M, NQK hd] from refs64_qk_norm.fwd64's namespace; rounded: a bf16 buffer (fp32 inputs otherwise)."""
    half = ref.hd // 2
    e = ref.y.abs() * (rstd_rel(ref.hd, not rounded) + 2.0 * U32)
    a, b, ea, eb, c, s = ref.y[..., :half], ref.y[..., half:], e[..., :half], e[..., half:], ref.c.abs(), ref.s.abs()
    out = ref.out.reshape(ref.y.shape).abs()
    lo = c * ea + s * eb + U32 * ((a * c).abs() + (b * s).abs() + out[..., :half])
    hi = c * eb + s * ea + U32 * ((b * c).abs() + (a * s).abs() + out[..., half:])
    bar = torch.cat([lo, hi], -1) + FP32_DENORM
    if rounded:
        bar = bar + BF16_OUT_REL * out
    return bar.reshape(ref.out.shape)


def bwd_bar(ref, cpu32, rounded):
    """Elementwise [M, NQK hd]: fp32_bar of the case (one number) + the bf16 rounding of the stored result."""
    bar = fp32_bar(ref.dx, cpu32.dx) + 0.0 * ref.dx.abs()
    return bar + BF16_OUT_REL * ref.dx.abs() if rounded else bar


def radial_bar(ref, hd, rounded):
    """Elementwise [M, NQK hd]: the absolute bound of the cancellation (derivation above), one value per (row, head)."""
    gmax, xmax = ref.g.abs().amax(-1, keepdim=True), ref.xh.abs().amax(-1, keepdim=True)
    bar = (hd + 4.0) * U32 * gmax * torch.clamp(xmax * xmax, min=1.0) * ref.rstd[..., None] + FP32_DENORM
    bar = bar.expand_as(ref.g).reshape(ref.dx.shape)
    return bar + BF16_OUT_REL * ref.dx.abs() if rounded else bar
