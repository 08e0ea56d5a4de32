"""The bar of avllm_lora_merge against float64 (tests/refs64_merge.py), derived as tests/bars.py derives its own: from the arithmetic the header
states, never from a kernel's output.

The kernel computes, in fp32, u = fma chain over j = 0 .. r-1 of B[n,j] * A[j,k] (ascending, from 0), then fl(scale * u + W) as one fma or as a
rounded product and a rounded sum, then one round-to-nearest-even to the storage type.

  * the chain: r fused steps, each rounding once.  The standard bound of a length-r recursive sum of products is gamma_r * sum_j |B||A| with
    gamma_r = r U32 / (1 - r U32), r U32 to first order (r <= 64: the second-order part is 4e-6 of the first).  Multiplied through by |scale| it is
    r * U32 * sum_abs with sum_abs = |scale| * sum_j |B[n,j]| |A[j,k]|, which refs64_merge.merge64 returns.
  * the product and the sum: U32 * |scale * u| for a separately rounded product plus U32 * |ref| for the rounded sum.  A contracted fma rounds once
    and is inside this.  For an f32 store that last rounding IS the store.
  * FP32_DENORM: a subnormal intermediate may be flushed.
  * a bf16 store rounds the fp32 result once more: BF16_OUT_REL * |ref| (2^-9 for the rounding, doubled for a tie moved by the fp32 error below).

The exact and locate families of tests/test_lora_merge_gpu.py have every intermediate and every result representable: their bar is 0."""
from bars import BF16_OUT_REL, FP32_DENORM, U32


def merge_bar(ref, u, sum_abs, r, scale, bf16_out):
    """Elementwise bar (float64 tensor like ref) of one merge: ref, u, sum_abs as refs64_merge.merge64 returns them."""
    bar = r * U32 * sum_abs + U32 * ((scale * u).abs() + ref.abs()) + FP32_DENORM
    if bf16_out:
        bar = bar + BF16_OUT_REL * ref.abs()
    return bar
