#!/usr/bin/env python3
"""Token-step time of the fused decode path at 7B shapes: bf16 weights against the weight-only fp8 stream (decode_fp8) and the weight-only fp4
stream (decode_fp4), alternated in one process: one engine holds all three weight forms and the descriptor's decode_fp8 / decode_fp4 flags
select the one a step reads.  Each step is a captured hipGraph replayed with the position in device memory (what generate() amortises), at a
cache position of 300 (bench.py's decode shape).  Synthetic weights; adapters (rank 16 on q, k, v, o) optional.  --model qwen2.5-7b runs
Qwen2.5-7B's shapes (d 3584, 28 heads over 4 kv heads, ffn 18944, vocab 152064, 28 layers) with its q|k|v biases.  Per form: the median over
the rounds and their spread (max - min); a difference between two forms counts only when it exceeds the spreads."""
import argparse, dataclasses, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import lib as L
from avllm import ops
from avllm.arch import LLAMA, LlamaCfg, LoraCfg
from avllm.engine import LlamaEngine

ap = argparse.ArgumentParser()
ap.add_argument("--model", choices=["llama2-7b", "mistral-7b", "qwen2.5-7b"], default="llama2-7b")
ap.add_argument("--batches", type=str, default="1,8,16")
ap.add_argument("--forms", type=str, default="bf16,fp8,fp4")
ap.add_argument("--lora", action="store_true")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--layers", type=int, default=0, help="fewer layers than the model's (32; Qwen2.5-7B: 28): a rehearsal, not a measurement")
a = ap.parse_args()
forms = a.forms.split(",")
assert forms and all(f in ("bf16", "fp8", "fp4") for f in forms), forms
dev, BF = "cuda:0", torch.bfloat16
if a.model == "qwen2.5-7b":
    cfg = dataclasses.replace(LLAMA["qwen2.5-7b"], layers=a.layers or LLAMA["qwen2.5-7b"].layers)
else:
    cfg = LlamaCfg(4096, 32, a.layers or 32, 11008, 32000) if a.model == "llama2-7b" else LlamaCfg(4096, 32, a.layers or 32, 14336, 32000, kv_heads=8)
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
        if nm.startswith("self_attn.") and (cfg.o_bias if nm.endswith("o_proj") else cfg.qkv_bias):
            sd[p + nm + ".bias"] = torch.randn(o, device=dev, generator=g, dtype=BF) * 0.3
    sd[p + "input_layernorm.weight"] = torch.ones(cfg.hidden, device=dev, dtype=BF)
    sd[p + "post_attention_layernorm.weight"] = torch.ones(cfg.hidden, device=dev, dtype=BF)
eng = LlamaEngine(sd, cfg, LoraCfg(16, 32.0) if a.lora else None, None, dtype=BF, device=dev, training=False, decode_fp8=True)
if "fp4" in forms:      # the fp4 images next to the fp8 ones (an engine built with decode_fp4=True holds them instead)
    for i in range(cfg.layers):
        p = f"model.layers.{i}."
        cat = lambda *ks: torch.cat([sd[p + k + ".weight"] for k in ks], 0)
        eng._fp4_images(eng.layers[i], cat("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), sd[p + "self_attn.o_proj.weight"],
                        cat("mlp.gate_proj", "mlp.up_proj"), sd[p + "mlp.down_proj.weight"])
del sd
if a.lora:
    eng.lora_p.normal_(0, 0.01)
    eng.pack_lora()
torch.cuda.synchronize()


def select(form):
    eng.desc.decode_fp8, eng.desc.decode_fp4 = int(form == "fp8"), int(form == "fp4")


def nbytes(form, B):
    select(form)
    return eng.streamed_weight_bytes(B)


print(f"{a.model}{' + adapters' if a.lora else ''}, {cfg.layers} layers: weight bytes per step " +
      ", ".join(f"{f} {nbytes(f, 8) / 1e9:.2f} GB" for f in forms), flush=True)


def graph(B, form):
    select(form)
    assert eng.decode_streams_fp8(B) == (form == "fp8") and eng.decode_streams_fp4(B) == (form == "fp4") and eng.decode_is_fused(B)
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
    gs = {f: graph(B, f) for f in forms}
    res = {f: [] for f in forms}
    for r in range(a.rounds):
        for f in forms:
            res[f].append(time_graph(*gs[f][:2]))
    med = {f: statistics.median(res[f]) for f in forms}
    line = f"B={B:2d}"
    for f in forms:
        line += f"  {f} {med[f]:.3f} ms +-{max(res[f]) - min(res[f]):.3f} ({nbytes(f, B) / med[f] / 1e9:.2f} TB/s)"
    for x, y in (("bf16", "fp8"), ("fp8", "fp4"), ("bf16", "fp4")):
        if x in med and y in med:
            line += f"  {x}/{y} {med[x] / med[y]:.2f}x"
    print(line + "  rounds " + " ".join(f"{f} {[round(x, 3) for x in res[f]]}" for f in forms), flush=True)
    del gs
    torch.cuda.empty_cache()
