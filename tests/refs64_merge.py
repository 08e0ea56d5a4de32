"""Float64 statement of the decode-time LoRA merge (csrc/lora_merge.hip, LlamaEngine.merge_lora) and the inputs its CPU file
(tests/test_merge_refs_cpu.py) and GPU files (tests/test_lora_merge_gpu.py, tests/test_generate_merged_gpu.py) share.  Everything is made from
seeds on the CPU; nothing here touches the GPU."""
import functools

import torch

import kv8_cases as K
from oracle import weights as Wt

F64 = torch.float64
TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj")
LORA_B_STD = 0.5         # at the usual 0.05 the adapters move the tiny model's logits by 0.6 %, below the bf16 bar: a dropped term would pass


def merge64(W, A, B, scale):
    """W [N,K], A [r,K], B [N,r] -> (W + scale * B.A, u = B.A, sum_abs = |scale| * |B|.|A|), float64."""
    W, A, B = W.to(F64), A.to(F64), B.to(F64)
    u = B @ A
    return W + scale * u, u, abs(scale) * (B.abs() @ A.abs())


def merged_sd64(sd, lora, layers, scale):
    """The state dict with every q/k/v/o weight replaced by its float64 merge (adapters as the oracle's `layers.N.<module>.lora_A|B` dict)."""
    out = dict(sd)
    for i in range(layers):
        for nm in TARGETS:
            key = f"model.layers.{i}.self_attn.{nm}.weight"
            out[key] = merge64(sd[key], lora[f"layers.{i}.{nm}.lora_A"], lora[f"layers.{i}.{nm}.lora_B"], scale)[0]
    return out


def bf16_round(sd):
    return {k: v.to(torch.bfloat16).float() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def tiny():
    """(oracle config at max_seq_len 256, weights) of kv8_cases.tiny() drawn again with adapters large enough to matter (LORA_B_STD) and the LLM
    base rounded to bf16 (what the bf16 engine holds); the adapters stay fp32, as the engine's masters are.  kv8_cases.greedy_inputs() are its
    inputs: the encoders and connectors do not depend on the adapters' draw."""
    oc, W0, _, _ = K.tiny()
    import numpy as np
    import os
    seed = int(np.load(os.path.join(K.GOLDEN, "g2_tiny_e2e.npz"))["seed"])
    W = Wt.all_weights(oc, seed, lora_b_std=LORA_B_STD)
    for k in ("whisper", "clip"):
        assert all(torch.equal(W[k][n], W0[k][n]) for n in W0[k])
    W["llama"] = bf16_round(W["llama"])
    return oc, W


def prefill_logits64(sd, lora, oc, x):
    """Logits of every position of the prefill [B, S, V], float64 (refs64_kv8.llama_hidden with an empty cache)."""
    import refs64_kv8 as R
    with torch.no_grad():
        h = R.llama_hidden(sd, lora, oc.llama, oc.lora if lora is not None else None, x, [None] * oc.llama.layers, 0, store=R.identity)
        return h @ sd["lm_head.weight"].to(F64).T
