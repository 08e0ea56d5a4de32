"""tests/mxfp4_ref.py against the published OCP MXFP4 rule: rounding ties and saturation, block exponents, the packed image, exactness in
bf16, and the format's error on Gaussian weights (printed for the record)."""
import torch

import mxfp4_ref as mx4

BF = torch.bfloat16


def _block(v, fill=0.0):
    """one 32-block whose amax is 4.0 (exponent 0, scale 1) holding v at element 1"""
    x = torch.full((1, 32), fill)
    x[0, 0] = 4.0
    x[0, 1] = v
    return x


def test_ties_go_to_the_even_code_and_large_values_saturate():
    table = [(0.25, 0, 0.0), (0.75, 2, 1.0), (1.25, 2, 1.0), (1.75, 4, 2.0), (2.5, 4, 2.0), (3.5, 6, 4.0), (5.0, 6, 4.0), (7.0, 7, 6.0)]
    for v, code, val in table:
        for sign in (1.0, -1.0):
            x = _block(sign * v)
            if v == 7.0:
                x[0, 0] = 7.5                                    # amax 7.5: exponent still 0, both elements saturate at 6
            codes, e = mx4.quantize(x)
            assert int(e[0, 0]) == 0
            assert int(codes[0, 1]) == (code | (8 if sign < 0 else 0)), (v, sign, int(codes[0, 1]))
            assert float(mx4.dequantize(codes, e)[0, 1]) == sign * val
    # off the ties: nearest
    for v, code in [(0.2, 0), (0.3, 1), (0.7, 1), (0.8, 2), (1.3, 3), (1.7, 3), (1.8, 4), (2.6, 5), (3.4, 5), (3.6, 6), (5.1, 7), (6.0, 7)]:
        assert int(mx4.quantize(_block(v))[0][0, 1]) == code, v
    # the same table at another scale: the rule is relative to the block's exponent
    codes, e = mx4.quantize(_block(1.25) * 2.0 ** -9)
    assert int(e[0, 0]) == -9 and int(codes[0, 1]) == 2 and int(codes[0, 0]) == 6


def test_exponents_zero_block_and_clamps():
    x = torch.zeros(1, 5 * 32)
    x[0, 32] = 1.0            # floor(log2) 0  -> -2
    x[0, 64] = 7.99           # 2 -> 0
    x[0, 96] = 2.0 ** -130    # subnormal: exponent field 0 -> clamped to -127
    x[0, 128] = 2.0 ** 127    # 127 - 2 = 125
    codes, e = mx4.quantize(x)
    assert e.tolist() == [[-127, -2, 0, -127, 125]]
    assert mx4.block_exponents(x).tolist() == e.tolist()
    assert int(codes[0, :32].max()) == 0                          # the zero block: all codes 0
    assert int(codes[0, 32]) == 6 and int(codes[0, 64]) == 7      # 1.0 * 2^2 = 4 -> code 6; 7.99 saturates at 6 -> code 7
    assert int(codes[0, 128]) == 6
    d = mx4.dequantize(codes, e)
    assert float(d[0, 32]) == 1.0 and float(d[0, 64]) == 6.0 and float(d[0, 128]) == 2.0 ** 127


def test_pack_puts_even_elements_in_the_low_nibble_and_round_trips():
    codes = torch.arange(64, dtype=torch.uint8).remainder(16).reshape(2, 32)
    img = mx4.pack(codes)
    assert img.shape == (2, 16) and img.dtype == torch.uint8
    assert int(img[0, 0]) == (0 | (1 << 4)) and int(img[0, 3]) == (6 | (7 << 4))
    assert torch.equal(mx4.unpack(img), codes)
    g = torch.Generator().manual_seed(3)
    W = torch.randn(24, 256, generator=g)
    c, e = mx4.quantize(W)
    assert torch.equal(mx4.unpack(mx4.pack(c)), c) and int(c.max()) < 16


def test_fake_quant_is_exact_in_bf16_and_idempotent():
    g = torch.Generator().manual_seed(4)
    for scale in (1.0, 4096 ** -0.5, 2.0 ** 40, 2.0 ** -60):
        W = torch.randn(64, 512, generator=g) * scale
        wt = mx4.fake_quant(W)
        assert torch.equal(wt.to(BF).float(), wt)
        assert torch.equal(mx4.fake_quant(wt), wt)


def test_relative_error_on_gaussian_weights_for_the_record():
    g = torch.Generator().manual_seed(0)
    W = torch.randn(512, 4096, generator=g) * 4096 ** -0.5
    err = float((mx4.fake_quant(W) - W).norm() / W.norm())
    print(f"MXFP4 round-to-nearest, randn(512, 4096) * 4096**-0.5: relative L2 error {err:.4f}")
    assert 0.0 < err < 1.0            # a sanity range, not a bar: the figure is for the record
