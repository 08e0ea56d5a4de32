#!/usr/bin/env python3
"""Token-step time of the fused decode path at 7B shapes, bf16 weights against the weight-only fp8 stream (decode_fp8), alternated in one
process: one engine holds both weight forms and the descriptor's decode_fp8 flag selects the one a step reads.  Each step is a captured
hipGraph replayed with the position in device memory (what generate() amortises), at a cache position of 300 (bench.py's decode shape).
Synthetic weights; adapters (rank 16 on q, k, v, o) optional."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import lib as L
from avllm import ops
from avllm.arch import LlamaCfg, LoraCfg
from avllm.engine import LlamaEngine

ap = argparse.ArgumentParser()
ap.add_argument("--model", choices=["llama2-7b", "mistral-7b"], default="llama2-7b")
ap.add_argument("--batches", type=str, default="1,8,16")
ap.add_argument("--lora", action="store_true")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
dev, BF = "cuda:0", torch.bfloat16
cfg = LlamaCfg(4096, 32, 32, 11008, 32000) if a.model == "llama2-7b" else LlamaCfg(4096, 32, 32, 14336, 32000, kv_heads=8)
g = torch.Generator(device=dev).manual_seed(0)
hd = cfg.hidden // cfg.heads
dkv = (cfg.kv_heads or cfg.heads) * hd


def w(o, k):
    return (torch.randn(o, k, device=dev, generator=g, dtype=BF) * k ** -0.5)


sd = {"model.embed_tokens.weight": w(cfg.vocab, cfg.hidden), "model.norm.weight": torch.ones(cfg.hidden, device=dev, dtype=BF),
      "lm_head.weight": w(cfg.vocab, cfg.hidden)}
for i in range(cfg.layers):
    p = f"model.layers.{i}."
    for nm, (o, k) in {"self_attn.q_proj": (cfg.hidden, cfg.hidden), "self_attn.k_proj": (dkv, cfg.hidden), "self_attn.v_proj": (dkv, cfg.hidden),
                       "self_attn.o_proj": (cfg.hidden, cfg.hidden), "mlp.gate_proj": (cfg.ffn, cfg.hidden), "mlp.up_proj": (cfg.ffn, cfg.hidden),
                       "mlp.down_proj": (cfg.hidden, cfg.ffn)}.items():
        sd[p + nm + ".weight"] = w(o, k)
    sd[p + "input_layernorm.weight"] = torch.ones(cfg.hidden, device=dev, dtype=BF)
    sd[p + "post_attention_layernorm.weight"] = torch.ones(cfg.hidden, device=dev, dtype=BF)
eng = LlamaEngine(sd, cfg, LoraCfg(16, 32.0) if a.lora else None, None, dtype=BF, device=dev, training=False, decode_fp8=True)
del sd
if a.lora:
    eng.lora_p.normal_(0, 0.01)
    eng.pack_lora()
torch.cuda.synchronize()
print(f"{a.model}{' + adapters' if a.lora else ''}: {eng.frozen_weight_bytes() / 1e9:.2f} GB bf16, {eng.streamed_weight_bytes(8) / 1e9:.2f} GB fp8 per step", flush=True)


def graph(B, fp8):
    eng.desc.decode_fp8 = int(fp8)
    assert eng.decode_streams_fp8(B) == fp8 and eng.decode_is_fused(B)
    kc, vc = eng.alloc_cache(B, 320 + a.steps + 8)
    ids = torch.randint(0, cfg.vocab, (B,), device=dev, generator=g)
    pd = torch.zeros(1, device=dev, dtype=torch.int32)
    out = torch.empty(B, cfg.vocab, device=dev, dtype=torch.float32)
    eng.decode_step(ids, 300, kc, vc, pos_dev=pd, logits=out)        # sizes the workspace outside the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(gr, stream=s):
        eng.decode_step(ids, 300, kc, vc, pos_dev=pd, logits=out)
        L.check(L.load().avllm_pos_advance(L.ptr(pd), 1, L.stream_ptr()))
    torch.cuda.current_stream().wait_stream(s)
    return gr, pd, (kc, vc, ids, out)


def time_graph(gr, pd):
    pd.zero_()
    for _ in range(3):
        gr.replay()
    pd.zero_()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        gr.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.steps


for B in [int(b) for b in a.batches.split(",")]:
    gs = {f: graph(B, f) for f in (False, True)}
    res = {False: [], True: []}
    for r in range(a.rounds):
        for f in (False, True):
            res[f].append(time_graph(*gs[f][:2]))
    eng.desc.decode_fp8 = 1
    nb = {f: (eng.frozen_weight_bytes() if not f else eng.streamed_weight_bytes(B)) for f in (False, True)}
    t16, t8 = min(res[False]), min(res[True])
    print(f"B={B:2d}  bf16 {t16:.3f} ms ({nb[False] / t16 / 1e9:.2f} TB/s of weights)   fp8 {t8:.3f} ms ({nb[True] / t8 / 1e9:.2f} TB/s)   "
          f"speed-up {t16 / t8:.2f}x   rounds bf16 {[round(x, 3) for x in res[False]]} fp8 {[round(x, 3) for x in res[True]]}", flush=True)
    del gs
    torch.cuda.empty_cache()
