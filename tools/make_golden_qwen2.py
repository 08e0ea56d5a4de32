#!/usr/bin/env python3
"""Write tests/golden/g12_attn_bias.npz (case "q") and g12_attn_bias_l.npz (case "l"): transformers' Qwen2ForCausalLM (biases on q, k, v) and LlamaForCausalLM(attention_bias=True) (biases
on q, k, v, o) on the CPU in fp32, with peft's lora.Linear (oracle/make_golden.py LoraLinear) around q/k/v/o, on the two models and batches of
tests/attn_bias_weights.py.  Per case ("q.", "l."): inputs_embeds, labels, logits, loss, every LoRA gradient, d loss / d inputs_embeds, eight
greedy tokens from generate(inputs_embeds=...), the logits of those eight steps, and the logits of the same eight positions with the adapters
switched off (teacher-forced on the same tokens: the token step without adapters has a reference too).  The weights are not stored: both sides draw them from
the seeded generator of tests/attn_bias_weights.py.  One file per case: the float32 arrays of both (1.2 MB, random mantissas do not compress)
do not fit one committed file.  Writes data, nothing else."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "audio-visual-llm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import attn_bias_weights as AW  # noqa: E402
from oracle.make_golden import LoraLinear  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-2


def build_hf(c, sd, lora):
    """The transformers model of case c (eager attention, fp32) with the LoRA modules in place (lora=None: the plain model)."""
    from transformers import LlamaConfig, LlamaForCausalLM, Qwen2Config, Qwen2ForCausalLM
    common = dict(hidden_size=c.hidden, intermediate_size=c.ffn, num_hidden_layers=c.layers, num_attention_heads=c.heads,
                  num_key_value_heads=c.kv_heads, vocab_size=c.vocab, rms_norm_eps=c.eps, max_position_embeddings=4096, rope_theta=c.theta,
                  tie_word_embeddings=False, attn_implementation="eager", pad_token_id=0, bos_token_id=1, eos_token_id=None)
    if c.o_bias:
        m = LlamaForCausalLM(LlamaConfig(attention_bias=True, **common))
    else:
        m = Qwen2ForCausalLM(Qwen2Config(use_sliding_window=False, **common))
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    for p in m.parameters():
        p.requires_grad_(False)
    if lora is None:
        return m.eval()
    scale = AW.ALPHA / AW.RANK
    for i, layer in enumerate(m.model.layers):
        for nm in ("q_proj", "k_proj", "v_proj", "o_proj"):
            base = getattr(layer.self_attn, nm)
            assert (base.bias is not None) == (c.o_bias if nm == "o_proj" else c.qkv_bias), nm
            setattr(layer.self_attn, nm, LoraLinear(base, lora[f"layers.{i}.{nm}.lora_A"], lora[f"layers.{i}.{nm}.lora_B"], scale))
    return m.eval()


def run_case(c, batch_seed=None):
    """dict of the case's arrays (no prefix), and the smallest top-2 margin over the greedy steps."""
    sd, lora = AW.weights(c)
    m = build_hf(c, sd, lora)
    x, labels = AW.batch(c, batch_seed)
    xg = x.clone().requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = m(inputs_embeds=xg, labels=labels)
        res.loss.backward()
        gen = m.generate(inputs_embeds=x, attention_mask=torch.ones(AW.B, AW.S, dtype=torch.long), max_new_tokens=AW.STEPS, do_sample=False,
                         output_scores=True, return_dict_in_generate=True, pad_token_id=0)
    out = {"inputs_embeds": x.numpy(), "labels": labels.numpy(), "logits": res.logits.detach().numpy(), "loss": res.loss.detach().numpy(),
           "dx_embeds": xg.grad.numpy().copy(), "tokens": gen.sequences.numpy(), "step_logits": torch.stack(gen.scores, 1).numpy()}
    mods = [getattr(layer.self_attn, nm) for layer in m.model.layers for nm in ("q_proj", "k_proj", "v_proj", "o_proj")]
    with torch.no_grad():
        seq = torch.cat([x, m.model.embed_tokens(gen.sequences[:, :-1])], 1)
        forced = m(inputs_embeds=seq).logits[:, AW.S - 1:]
        assert float((forced - torch.stack(gen.scores, 1)).abs().max()) < 1e-4      # teacher forcing reproduces the cached steps
        for mod in mods:
            mod.scale = 0.0
        out["step_logits_base"] = m(inputs_embeds=seq).logits[:, AW.S - 1:].numpy()
    assert out["tokens"].shape == (AW.B, AW.STEPS) and out["step_logits"].shape == (AW.B, AW.STEPS, c.vocab)
    for i, layer in enumerate(m.model.layers):
        for nm in ("q_proj", "k_proj", "v_proj", "o_proj"):
            mod = getattr(layer.self_attn, nm)
            out[f"grad.layers.{i}.{nm}.lora_A"] = mod.lora_A.grad.numpy().copy()
            out[f"grad.layers.{i}.{nm}.lora_B"] = mod.lora_B.grad.numpy().copy()
    top = torch.stack(gen.scores, 1).topk(2, -1).values
    return out, float((top[..., 0] - top[..., 1]).min())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    for c in AW.CASES.values():
        # the batch seed recorded in attn_bias_weights.CASES was picked with this scan: the first one whose eight greedy steps all have a clear winner
        if "--scan" in sys.argv:
            for s in range(32):
                _, margin = run_case(c, s)
                print(f"case {c.name} batch seed {s}: smallest top-2 margin {margin:.4f}")
                if margin >= MARGIN:
                    break
            continue
        arrays, margin = run_case(c)
        print(f"case {c.name}: loss {float(arrays['loss']):.6f}, smallest top-2 margin over {AW.STEPS} greedy steps {margin:.4f}")
        assert margin >= MARGIN, f"case {c.name}: a greedy step is decided by {margin}: pick another batch seed (--scan)"
        path = os.path.join(GOLDEN, AW.golden_name(c))
        np.savez_compressed(path, **{f"{c.name}.{k}": v for k, v in arrays.items()})
        size = os.path.getsize(path)
        print("wrote", path, size, "bytes")
        assert size < os.path.getsize(os.path.join(GOLDEN, "g2_tiny_e2e.npz")) and size < 1 << 20, size


if __name__ == "__main__":
    main()
