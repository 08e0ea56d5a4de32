"""CPU restatement of OCP MXFP4 (Microscaling v1.0: e2m1 elements, one E8M0 scale per 32 consecutive elements along K), the weight format
of the fp4 token step (csrc/fp4.hip, csrc/decode.hip).  It restates the published rule, as oracle/mxfp8.py does for e4m3, with emax = 2:

  e     = floor(log2(amax of the block)) - 2, clamped to [-127, 127]; an all-zero block gets -127
  value = x * 2^-e rounded to nearest, ties to the even code, onto {0, 0.5, 1, 1.5, 2, 3, 4, 6}; saturated at +-6
  code  = sign << 3 | index of |value| in that grid        (sign = x < 0)
  image = uint8 [..., K/2]: element 2i in the low nibble of byte i, element 2i + 1 in the high nibble

Every dequantised value (grid value * 2^e) is exactly a bf16 value, so fake_quant(W) is an ordinary bf16 weight set."""
from __future__ import annotations

import torch

BLOCK = 32
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
# decision points between neighbouring codes; a tie goes to the even code: `>` where the lower neighbour is even, `>=` where it is odd
_BOUNDS = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False), (3.5, True), (5.0, False))


def block_exponents(x: torch.Tensor) -> torch.Tensor:
    """x [..., K] (K % 32 == 0) -> int32 exponents [..., K/32]."""
    xb = x.float().reshape(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    bits = xb.abs().amax(-1).contiguous().view(torch.int32)
    e = ((bits >> 23) & 0xFF) - 127 - 2            # exponent field: floor(log2) for normal numbers; 0 / subnormal -> clamped below
    return e.clamp(-127, 127).to(torch.int32)


def round_e2m1(a: torch.Tensor) -> torch.Tensor:
    """a >= 0 (already scaled) -> index 0..7 into GRID, round to nearest even, saturating."""
    idx = torch.zeros(a.shape, dtype=torch.int32)
    for b, inclusive in _BOUNDS:
        idx += (a >= b).to(torch.int32) if inclusive else (a > b).to(torch.int32)
    return idx


def quantize(x: torch.Tensor):
    """-> (codes uint8 [..., K], one 4-bit code per element, unpacked; exponents int32 [..., K/32])."""
    x = x.float()
    e = block_exponents(x)
    inv = torch.ldexp(torch.ones((), dtype=torch.float32), -e)                    # 2^-e (e <= 125 for finite x)
    xb = x.reshape(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    idx = round_e2m1(xb.abs() * inv.unsqueeze(-1))
    codes = idx | ((xb < 0).to(torch.int32) << 3)
    return codes.to(torch.uint8).reshape(x.shape), e


def dequantize(codes: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """codes uint8 [..., K] (unpacked), e int32 [..., K/32] -> float32 [..., K]."""
    c = codes.to(torch.int64)
    v = GRID[c & 7] * torch.where((c & 8) != 0, -1.0, 1.0)
    v = v.reshape(*codes.shape[:-1], codes.shape[-1] // BLOCK, BLOCK)
    return (v * torch.ldexp(torch.ones((), dtype=torch.float32), e.to(torch.int32)).unsqueeze(-1)).reshape(codes.shape)


def fake_quant(x: torch.Tensor) -> torch.Tensor:
    return dequantize(*quantize(x))


def pack(codes: torch.Tensor) -> torch.Tensor:
    """codes uint8 [..., K] -> image uint8 [..., K/2]: element 2i in the low nibble."""
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).contiguous()


def unpack(img: torch.Tensor) -> torch.Tensor:
    return torch.stack([img & 15, img >> 4], -1).reshape(*img.shape[:-1], 2 * img.shape[-1])
