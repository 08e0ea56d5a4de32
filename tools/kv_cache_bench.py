#!/usr/bin/env python3
"""Token-step time of the fused decode path with the bf16 KV cache against the fp8 one (kv_cache="fp8": block-scaled e4m3 rows, csrc/kv_fp8.hip),
in tools/decode_step_bench.py's style: 7B shapes, synthetic weights, one engine that holds the bf16, fp8 and fp4 weight forms, every
(weights, cache) form a captured hipGraph of one step replayed with the position in device memory, all forms of one (rows, prefix) cell
alternated in one process.  Per form the median over the rounds and their spread (max - min); a difference counts only when it exceeds the spreads.
The bf16-cache leg is the path decode_step_bench.py times (there at cache position 300: --prefixes 300 makes the two comparable).
--attention: the attention launch alone at 16 rows, one launch per layer over 32 distinct caches (so no launch finds its rows in the last-level
cache), both forms: time per launch and achieved bytes/s.
--accuracy: relative L2 of the step logits, fp8 cache against bf16 cache, on a 2-layer model of the same width after 48 forced steps."""
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
ap.add_argument("--prefixes", type=str, default="256,544")
ap.add_argument("--weights", type=str, default="bf16,fp8,fp4")
ap.add_argument("--lora", action="store_true")
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--layers", type=int, default=0, help="fewer layers than the model's: a rehearsal, not a measurement")
ap.add_argument("--attention", action="store_true")
ap.add_argument("--accuracy", action="store_true")
a = ap.parse_args()
wforms = a.weights.split(",")
assert wforms and all(f in ("bf16", "fp8", "fp4") for f in wforms), wforms
dev, BF = "cuda:0", torch.bfloat16
if a.model == "qwen2.5-7b":
    cfg = dataclasses.replace(LLAMA["qwen2.5-7b"], layers=a.layers or LLAMA["qwen2.5-7b"].layers)
else:
    cfg = LlamaCfg(4096, 32, a.layers or 32, 11008, 32000) if a.model == "llama2-7b" else LlamaCfg(4096, 32, a.layers or 32, 14336, 32000, kv_heads=8)
g = torch.Generator(device=dev).manual_seed(0)
hd = cfg.hidden // cfg.heads
kvh = cfg.kv_heads or cfg.heads
dkv = kvh * hd


def fill(cache):
    """Finite rows in either form (timing does not read them as numbers, but NaN codes should not be what is measured)."""
    if cache.dtype == torch.uint8:
        q, e = ops.kv8_unpack(cache)
        q.copy_(torch.randint(0, 0x7F, q.shape, device=dev, generator=g, dtype=torch.uint8))
        e.copy_(torch.randint(118, 124, e.shape, device=dev, generator=g, dtype=torch.uint8))
    else:
        cache.normal_(0, 1, generator=g)


def build(layers):
    c = dataclasses.replace(cfg, layers=layers)
    w = lambda o, k: torch.randn(o, k, device=dev, generator=g, dtype=BF) * k ** -0.5  # noqa: E731
    sd = {"model.embed_tokens.weight": w(c.vocab, c.hidden), "model.norm.weight": torch.ones(c.hidden, device=dev, dtype=BF), "lm_head.weight": w(c.vocab, c.hidden)}
    for i in range(c.layers):
        p = f"model.layers.{i}."
        for nm, (o, k) in {"self_attn.q_proj": (c.hidden, c.hidden), "self_attn.k_proj": (dkv, c.hidden), "self_attn.v_proj": (dkv, c.hidden),
                           "self_attn.o_proj": (c.hidden, c.hidden), "mlp.gate_proj": (c.ffn, c.hidden), "mlp.up_proj": (c.ffn, c.hidden),
                           "mlp.down_proj": (c.hidden, c.ffn)}.items():
            sd[p + nm + ".weight"] = w(o, k)
            if nm.startswith("self_attn.") and (c.o_bias if nm.endswith("o_proj") else c.qkv_bias):
                sd[p + nm + ".bias"] = torch.randn(o, device=dev, generator=g, dtype=BF) * 0.3
        sd[p + "input_layernorm.weight"] = torch.ones(c.hidden, device=dev, dtype=BF)
        sd[p + "post_attention_layernorm.weight"] = torch.ones(c.hidden, device=dev, dtype=BF)
    eng = LlamaEngine(sd, c, LoraCfg(16, 32.0) if a.lora else None, None, dtype=BF, device=dev, training=False, decode_fp8=True, kv_fp8=True)
    if "fp4" in wforms:
        for i in range(c.layers):
            p = f"model.layers.{i}."
            cat = lambda *ks: torch.cat([sd[p + k + ".weight"] for k in ks], 0)  # noqa: E731
            eng._fp4_images(eng.layers[i], cat("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), sd[p + "self_attn.o_proj.weight"],
                            cat("mlp.gate_proj", "mlp.up_proj"), sd[p + "mlp.down_proj.weight"])
    if a.lora:
        eng.lora_p.normal_(0, 0.01)
        eng.pack_lora()
    torch.cuda.synchronize()
    return eng


def select(eng, form):
    eng.desc.decode_fp8, eng.desc.decode_fp4 = int(form == "fp8"), int(form == "fp4")


def accuracy():
    eng = build(2)
    select(eng, "bf16")
    B, S, new = 8, 256, 48
    x = torch.randn(B, S, cfg.hidden, device=dev, generator=g, dtype=BF) * 0.5
    ids = torch.randint(0, cfg.vocab, (B, new), device=dev, generator=g)
    outs = {}
    for form in ("bf16", "fp8"):
        kc, vc = eng.alloc_cache(B, S + new, fp8=form == "fp8")
        eng.prefill(x, kc, vc)
        outs[form] = torch.stack([eng.decode_step(ids[:, t].contiguous(), S + t, kc, vc).clone() for t in range(new)], 1).double()
    rl2 = lambda x_, y_: float(((x_ - y_) ** 2).sum().sqrt() / (y_ ** 2).sum().sqrt())  # noqa: E731
    print(f"accuracy: {a.model} width, 2 layers, {B} rows, prefix {S}, {new} forced steps: step logits, fp8 cache against bf16 cache, relative L2 "
          f"{rl2(outs['fp8'], outs['bf16']):.3e} over all steps, {rl2(outs['fp8'][:, -1], outs['bf16'][:, -1]):.3e} at step {new}; "
          f"argmax equal at {float((outs['fp8'].argmax(-1) == outs['bf16'].argmax(-1)).double().mean()):.3f} of the {B * new} rows", flush=True)


def attention(B=16, P=544, reps=20):
    nl, Tk, Tmax = 32, P + 1, P + 8
    q = torch.randn(B, cfg.hidden, device=dev, generator=g, dtype=BF)
    res = {}
    for form in ("bf16", "fp8"):
        if form == "fp8":
            caches = [(ops.kv8_alloc(B, Tmax, dkv=dkv, device=dev), ops.kv8_alloc(B, Tmax, dkv=dkv, device=dev)) for _ in range(nl)]
            run = lambda kc, vc: ops.attention_decode_kv8(q, kc, vc, cfg.heads, Tk)  # noqa: E731
        else:
            caches = [(torch.empty(B, Tmax, dkv, device=dev, dtype=BF), torch.empty(B, Tmax, dkv, device=dev, dtype=BF)) for _ in range(nl)]
            run = lambda kc, vc: ops.attention_decode(q, kc, vc, cfg.heads, Tk)  # noqa: E731
        for kc, vc in caches:
            fill(kc); fill(vc)
        times = []
        for r in range(a.rounds + 1):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                for kc, vc in caches:
                    run(kc, vc)
            e1.record(); torch.cuda.synchronize()
            if r:                                               # round 0 warms up
                times.append(e0.elapsed_time(e1) * 1e3 / (reps * nl))
        nbytes = 2 * B * Tk * dkv * (33 / 32 if form == "fp8" else 2)
        res[form] = (statistics.median(times), max(times) - min(times), nbytes)
        del caches
        torch.cuda.empty_cache()
    line = f"attention launch alone, {a.model}: {B} rows x {cfg.heads} heads over {kvh} kv heads, {Tk} cache rows, back-to-back launches over {nl} distinct caches:"
    for form, (med, spread, nbytes) in res.items():
        line += f"  {form} cache {med:.1f} us +-{spread:.1f} ({nbytes / 1e6:.1f} MB, {nbytes / med / 1e6:.2f} TB/s)"
    print(line + f"  bf16/fp8 {res['bf16'][0] / res['fp8'][0]:.2f}x", flush=True)


if a.accuracy:
    accuracy()
if a.attention:
    attention()
if a.accuracy or a.attention:
    sys.exit(0)

eng = build(cfg.layers)
print(f"{a.model}{' + adapters' if a.lora else ''}, {cfg.layers} layers, dkv {dkv}; {a.steps} steps per round, {a.rounds} rounds, forms alternated", flush=True)


def graph(B, P, wform, cform):
    select(eng, wform)
    assert eng.decode_streams_fp8(B) == (wform == "fp8") and eng.decode_streams_fp4(B) == (wform == "fp4") and eng.decode_is_fused(B)
    assert eng.decode_caches_fp8(B)
    kc, vc = eng.alloc_cache(B, P + a.steps + 8, fp8=cform == "fp8")
    fill(kc); fill(vc)
    ids = torch.randint(0, cfg.vocab, (B,), device=dev, generator=g)
    pd = torch.zeros(1, device=dev, dtype=torch.int32)
    out = torch.empty(B, cfg.vocab, device=dev, dtype=torch.float32)
    eng.decode_step(ids, P, kc, vc, pos_dev=pd, logits=out)          # sizes the workspace outside the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(gr, stream=s):
        eng.decode_step(ids, P, kc, vc, pos_dev=pd, logits=out)
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
    for P in [int(p) for p in a.prefixes.split(",")]:
        forms = [(w, c) for w in wforms for c in ("bf16", "fp8")]
        gs = {f: graph(B, P, *f) for f in forms}
        res = {f: [] for f in forms}
        for r in range(a.rounds):
            for f in forms:
                select(eng, f[0])
                res[f].append(time_graph(*gs[f][:2]))
        med = {f: statistics.median(res[f]) for f in forms}
        mb = {c: eng.kv_cache_bytes(B, P + 1, fp8=c == "fp8") / 1e6 for c in ("bf16", "fp8")}
        line = f"B={B:2d} prefix={P:3d} (cache read per step {mb['bf16']:.0f} -> {mb['fp8']:.0f} MB)"
        for w in wforms:
            x, y = (w, "bf16"), (w, "fp8")
            line += (f"  weights {w}: bf16 cache {med[x]:.3f} ms +-{max(res[x]) - min(res[x]):.3f}, fp8 cache {med[y]:.3f} ms +-{max(res[y]) - min(res[y]):.3f},"
                     f" {med[x] / med[y]:.3f}x")
        print(line, flush=True)
        del gs
        torch.cuda.empty_cache()
