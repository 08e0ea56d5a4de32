"""Error bars for the acoustic augmentation kernels, each derived from the roundings the rule of include/avllm.h prescribes; none comes from a
kernel's output.  u32 = 2^-24 and u64 = 2^-53 are the unit roundoffs of float32 and float64.

Integer outputs (applied, row, offset, spans), the recorded snr_db (a stated sequence of IEEE operations, restated bit for bit) and every copied
or unmasked cell carry a bar of 0: they are compared by bits."""
import math

import numpy as np

U32, U64 = 2.0 ** -24, 2.0 ** -53
F32_TINY = 2.0 ** -149          # one rounding that lands in the subnormals errs by at most half of this


def gain_bar(g, n):
    """|gain - g| for g = sqrt(Es / (En 10^(snr/10))) from exactly rounded energies.
    - The squares of float32 values are exact in double.  A double sum of n non-negative terms in ANY fixed order has a relative error of at
      most (n - 1) u64 / (1 - (n - 1) u64) (Higham, Accuracy and Stability, eq. 4.4: every partial sum is itself bounded by the total); the
      reference sum (math.fsum) adds one rounding: n u64 covers each energy to first order, doubled below for the second-order terms.
    - snr / 10, pow, the product, the quotient and the square root: five double operations, pow allowed 2 ulp (the accuracy ocml and glibc
      both document for it is within 1 ulp; 2 leaves room), the others correctly rounded.  pow amplifies the error of its argument by
      |snr / 10| ln 10 <= 7 for |snr| <= 30 dB.  Together (1 + 7 + 4 + 1 + 1 + 1) u64 at most: 16 u64.
    - The square root halves the relative error of its argument; this bar does not take that credit.
    - One double -> float rounding: u32 relative (the gains here are far from the subnormals)."""
    return abs(g) * (U32 + (4 * n + 16) * U64)


def mix_bar(w, z, g, n):
    """Per sample |out_i - (w_i + g z_i)| with g the float64 gain: the kernel's gain differs from g by at most gain_bar, which moves the
    product by |z_i| gain_bar; the product is rounded once (u32 |g z_i|) and the sum once (u32 |w_i + g z_i|); each rounding acts on a value
    already off by the earlier ones, a factor of (1 + 2^-20) covers that with room; a result in the subnormals errs by F32_TINY / 2 per
    rounding."""
    w, z = np.asarray(w, dtype=np.float64), np.asarray(z, dtype=np.float64)
    gz = g * z
    return (np.abs(z) * gain_bar(g, n) + U32 * (np.abs(gz) + np.abs(w + gz))) * (1.0 + 2.0 ** -20) + F32_TINY


def snr_bar_db(w, z, g, n):
    """|achieved - requested| in dB, achieved = 10 log10(Es / sum (out - w)^2) in float64.  g z is the noise that gives the requested SNR
    exactly; the kernel's out - w differs from it per sample by at most mix_bar, so ||out - w|| / ||g z|| lies in [1 - r, 1 + r] with
    r = ||mix_bar|| / ||g z|| (triangle inequality in l2), and the SNR moves by at most -20 log10(1 - r) dB (the larger side).  g itself
    stands for the exact gain up to a relative 16 u64 + 4 n u64 (gain_bar without the float rounding), which is inside r's first term.  The
    float64 evaluation of the achieved SNR adds a few u64: 1e-12 dB covers it."""
    gz = g * np.asarray(z, dtype=np.float64)
    r = math.sqrt(float(np.sum(mix_bar(w, z, g, n) ** 2))) / math.sqrt(float(np.sum(gz * gz)))
    return (-20.0 * math.log10(1.0 - r) if r < 1.0 else math.inf) + 1e-12


def bits(x):
    """float32 array -> its bit patterns: the comparison for bar 0 (NaN payloads and -0 count)."""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
