"""The inputs the kv_cache="fp8" tests share between their CPU file (tests/test_kv8_refs_cpu.py: the reference's own decisions on these inputs are
clear often enough for the comparison to say something) and their GPU file (tests/test_generate_kv8_gpu.py: generate() is followed against that
reference).  Everything is made from seeds on the CPU; nothing here touches the GPU."""
import functools
import os

import numpy as np
import torch

from oracle import avsr_oracle as O
from oracle import weights as Wt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_GREEDY = 24            # new tokens of the greedy runs (as test_generate_bf16_fused_token_step_vs_oracle_greedy)
MIN_HELD = 8             # decisions every comparison must hold the implementation to
# beam search: 2 items x 3 beams, EOS 53 (a token the tiny model's decode emits early: tests/test_generate_beam_gpu.py), 8 new tokens
BEAM_B, BEAM_NB, BEAM_N, BEAM_EOS = 2, 3, 8, 53
QWEN3_NEW = 16


def threshold():
    from bars import BF16_LOGIT_MAX_ABS
    return 2.0 * BF16_LOGIT_MAX_ABS


@functools.lru_cache(maxsize=None)
def tiny(with_lora=True):
    """(oracle config at max_seq_len 256, weights) of the reference-pinned tiny model (tests/golden/g2_tiny_e2e.npz)."""
    g = np.load(os.path.join(GOLDEN, "g2_tiny_e2e.npz"))
    oc = Wt.tiny()
    oc.max_seq_len = 256
    W = Wt.all_weights(oc, int(g["seed"]), lora_b_std=0.05)
    if not with_lora:
        W = {k: v for k, v in W.items() if k != "lora"}
    return oc, W, int(g["frames"]), int(g["batch_seed"])


@functools.lru_cache(maxsize=None)
def greedy_inputs():
    """(audio, video, LLM inputs x [4, S, d] as the oracle computes them) of the golden batch."""
    oc, W, frames, batch_seed = tiny()
    audio, video, _, _ = Wt.synthetic_batch(oc, 4, frames, seed=batch_seed)
    with torch.no_grad():
        x, _ = O.encode(W, oc, audio, video, None)
    return audio, video, x


@functools.lru_cache(maxsize=None)
def beam_inputs():
    """The first BEAM_B items of the golden batch."""
    audio, video, x = greedy_inputs()
    return audio[:BEAM_B], video[:BEAM_B], x[:BEAM_B]


def qwen3_inputs():
    """(case, weights, adapters, inputs_embeds [B, S, d]) of Qwen3 case "a" of tests/qwen3_weights.py, every tensor rounded to bf16 (what the
    bf16 engine holds), as float32."""
    import qwen3_weights as QW
    c = QW.CASES["a"]
    sd, lora = ({k: v.to(torch.bfloat16).float() for k, v in t.items()} for t in QW.weights(c))
    return c, sd, lora, QW.batch(c)[0]
