"""What the code-form token steps multiply, as ordinary state dicts on the host: every frozen projection (and lm_head) of an HF-named state
dict replaced by W~ = dequantize(quantize(W)) of its form (oracle/mxfp8.py for e4m3, tests/mxfp4_ref.py for MXFP4).  W~ is exactly a bf16
weight set, so a bf16 engine or a float64 reference built from these dicts computes what decode_fp8 / decode_fp4 compute on the codes."""
import torch

import mxfp4_ref as mx4
from oracle import mxfp8

BF = torch.bfloat16
PROJ = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def dequantised(sd):
    """The state dict with every frozen projection and lm_head replaced by W~ (what the fp8 token step multiplies)."""
    out = dict(sd)
    for k, v in sd.items():
        if k == "lm_head.weight" or any(k.endswith(p + ".weight") for p in PROJ):
            out[k] = mxfp8.fake_quant(v.to(BF).float())
    return out


def dequantised4(sd):
    """The state dict with every frozen projection replaced by its MXFP4 W~ and lm_head by its e4m3 W~ (what the fp4 token step multiplies)."""
    out = dict(sd)
    for k, v in sd.items():
        if k == "lm_head.weight":
            out[k] = mxfp8.fake_quant(v.to(BF).float())
        elif any(k.endswith(p + ".weight") for p in PROJ):
            out[k] = mx4.fake_quant(v.to(BF).float())
    return out
