#!/usr/bin/env python3
"""Token-step time of the fused decode path with every beam reading its own copy of the prefix (generate()'s default: an R-row cache of
prefix + generated positions) against the shared form (share_prefix=True: one B-row prefix cache, an R-row suffix cache;
csrc/attention_decode_shared.hip), in tools/kv_cache_bench.py's style: 7B shapes, synthetic weights, one engine that holds the bf16 and fp4
weight forms and both cache forms, every (weights, cache, copy | shared) form a captured hipGraph of one step replayed with the position in
device memory, all forms of one (items x group, prefix) cell alternated in one process.  Per form the median over the rounds and their spread
(max - min); a difference counts only when it exceeds the spreads.  Also per cell: the attention launch(es) of one layer alone (a graph of one
launch per layer over 32 distinct caches, at --new / 2 generated positions) and the KV bytes allocated for --new generated positions.
--prefill: the prefill of B rows against B * n rows (what sampled n-best saves when it shares)."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import lib as L
from avllm import ops
from avllm.arch import LlamaCfg
from avllm.engine import LlamaEngine

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=str, default="4x4,2x8,16x1,1x4", help="items x group")
ap.add_argument("--prefixes", type=str, default="256,544,1500")
ap.add_argument("--weights", type=str, default="bf16,fp4")
ap.add_argument("--caches", type=str, default="bf16,fp8")
ap.add_argument("--new", type=int, default=100, help="generated positions the caches are sized for")
ap.add_argument("--steps", type=int, default=48)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--layers", type=int, default=0, help="fewer layers than the model's: a rehearsal, not a measurement")
ap.add_argument("--prefill", action="store_true")
a = ap.parse_args()
wforms, cforms = a.weights.split(","), a.caches.split(",")
assert all(f in ("bf16", "fp8", "fp4") for f in wforms) and all(c in ("bf16", "fp8") for c in cforms) and a.steps <= a.new
dev, BF = "cuda:0", torch.bfloat16
cfg = LlamaCfg(4096, 32, a.layers or 32, 11008, 32000)
g = torch.Generator(device=dev).manual_seed(0)
hd = cfg.hidden // cfg.heads
dkv = (cfg.kv_heads or cfg.heads) * hd


def fill(cache):
    """Finite rows in either form (timing does not read them as numbers, but NaN codes should not be what is measured)."""
    if cache.dtype == torch.uint8:
        q, e = ops.kv8_unpack(cache)
        q.copy_(torch.randint(0, 0x7F, q.shape, device=dev, generator=g, dtype=torch.uint8))
        e.copy_(torch.randint(118, 124, e.shape, device=dev, generator=g, dtype=torch.uint8))
    else:
        cache.normal_(0, 1, generator=g)
    return cache


def build():
    c = cfg
    w = lambda o, k: torch.randn(o, k, device=dev, generator=g, dtype=BF) * k ** -0.5  # noqa: E731
    sd = {"model.embed_tokens.weight": w(c.vocab, c.hidden), "model.norm.weight": torch.ones(c.hidden, device=dev, dtype=BF), "lm_head.weight": w(c.vocab, c.hidden)}
    for i in range(c.layers):
        p = f"model.layers.{i}."
        for nm, (o, k) in {"self_attn.q_proj": (c.hidden, c.hidden), "self_attn.k_proj": (dkv, c.hidden), "self_attn.v_proj": (dkv, c.hidden),
                           "self_attn.o_proj": (c.hidden, c.hidden), "mlp.gate_proj": (c.ffn, c.hidden), "mlp.up_proj": (c.ffn, c.hidden),
                           "mlp.down_proj": (c.hidden, c.ffn)}.items():
            sd[p + nm + ".weight"] = w(o, k)
        sd[p + "input_layernorm.weight"] = torch.ones(c.hidden, device=dev, dtype=BF)
        sd[p + "post_attention_layernorm.weight"] = torch.ones(c.hidden, device=dev, dtype=BF)
    eng = LlamaEngine(sd, c, None, None, dtype=BF, device=dev, training=False, decode_fp8=True, kv_fp8=True)
    if "fp4" in wforms:
        for i in range(c.layers):
            p = f"model.layers.{i}."
            cat = lambda *ks: torch.cat([sd[p + k + ".weight"] for k in ks], 0)  # noqa: E731
            eng._fp4_images(eng.layers[i], cat("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), sd[p + "self_attn.o_proj.weight"],
                            cat("mlp.gate_proj", "mlp.up_proj"), sd[p + "mlp.down_proj.weight"])
    torch.cuda.synchronize()
    return eng


def select(eng, form):
    eng.desc.decode_fp8, eng.desc.decode_fp4 = int(form == "fp8"), int(form == "fp4")


def capture(fn):
    fn()                                                        # sizes workspaces outside the capture
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s), torch.cuda.graph(gr, stream=s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    return gr


def time_replays(gr, n, before=lambda: None):
    before()
    for _ in range(3):
        gr.replay()
    before()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        gr.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n                              # ms per replay


eng = build()
print(f"llama2-7b shapes, {cfg.layers} layers, dkv {dkv}; {a.steps} steps per round, {a.rounds} rounds, forms alternated; caches sized for {a.new} new positions",
      flush=True)


def step_graph(B, group, P, wform, cform, shared):
    """One token step of R = B group rows, the position in device memory: copy form at cache position P + *pd, shared form at suffix row *pd."""
    R, fp8 = B * group, cform == "fp8"
    select(eng, wform)
    assert eng.decode_is_fused(R) and eng.decode_shares_prefix(R) and eng.decode_streams_fp4(R) == (wform == "fp4")
    ids = torch.randint(0, cfg.vocab, (R,), device=dev, generator=g)
    pd = torch.zeros(1, device=dev, dtype=torch.int32)
    out = torch.empty(R, cfg.vocab, device=dev, dtype=torch.float32)
    if shared:
        kp, vp = (fill(t) for t in eng.alloc_cache(B, P, fp8=fp8))
        ks, vs = (fill(t) for t in eng.alloc_cache(R, a.new, fp8=fp8))
        keep = (kp, vp, ks, vs, ids, out)
        run = lambda: eng.decode_step_shared(ids, 0, kp, vp, ks, vs, group, pos_dev=pd, logits=out)  # noqa: E731
    else:
        kc, vc = (fill(t) for t in eng.alloc_cache(R, P + a.new, fp8=fp8))
        keep = (kc, vc, ids, out)
        run = lambda: eng.decode_step(ids, P, kc, vc, pos_dev=pd, logits=out)  # noqa: E731

    def both():
        run()
        L.check(L.load().avllm_pos_advance(L.ptr(pd), 1, L.stream_ptr()))
    return capture(both), pd, keep


def attention_graph(B, group, P, cform, shared, nl=32):
    """The attention launch(es) of one layer, once per each of nl distinct caches (no launch finds its rows in the last-level cache)."""
    R, fp8, n = B * group, cform == "fp8", a.new // 2
    q = torch.randn(R, cfg.hidden, device=dev, generator=g, dtype=BF)
    mk = (lambda rows, T: fill(ops.kv8_alloc(rows, T, dkv=dkv, device=dev))) if fp8 else (lambda rows, T: fill(torch.empty(rows, T, dkv, device=dev, dtype=BF)))
    if shared:
        caches = [(mk(B, P), mk(B, P), mk(R, a.new), mk(R, a.new)) for _ in range(nl)]
        f = ops.attention_decode_shared_kv8 if fp8 else ops.attention_decode_shared
        run = lambda c: f(q, c[0], c[1], P, c[2], c[3], cfg.heads, n, group)  # noqa: E731
    else:
        caches = [(mk(R, P + a.new), mk(R, P + a.new)) for _ in range(nl)]
        f = ops.attention_decode_kv8 if fp8 else ops.attention_decode
        run = lambda c: f(q, c[0], c[1], cfg.heads, P + n + 1)  # noqa: E731

    def all_layers():
        for c in caches:
            run(c)
    return capture(all_layers), caches, nl


def spread(xs):
    return max(xs) - min(xs)


for cell in a.cells.split(","):
    B, group = (int(x) for x in cell.split("x"))
    R = B * group
    for P in [int(p) for p in a.prefixes.split(",")]:
        for cform in cforms:
            fp8 = cform == "fp8"
            copy_b = eng.kv_cache_bytes(R, P + a.new, fp8=fp8)
            shared_b = eng.kv_cache_bytes(B, P, fp8=fp8) + eng.kv_cache_bytes(R, a.new, fp8=fp8)
            line = f"{B:2d}x{group} prefix={P:4d} cache {cform:4s} KV {copy_b / 2 ** 20:7.0f} -> {shared_b / 2 ** 20:7.0f} MiB |"
            ag = {sh: attention_graph(B, group, P, cform, sh) for sh in (False, True)}
            at = {sh: [] for sh in ag}
            for r in range(a.rounds):
                for sh, (gr, _, nl) in ag.items():
                    at[sh].append(time_replays(gr, 10) * 1e3 / nl)
            line += (f" attention copy {statistics.median(at[False]):5.1f} us +-{spread(at[False]):.1f}, shared {statistics.median(at[True]):5.1f} us "
                     f"+-{spread(at[True]):.1f} |")
            del ag
            torch.cuda.empty_cache()
            forms = [(w, sh) for w in wforms for sh in (False, True)]
            gs = {f: step_graph(B, group, P, f[0], cform, f[1]) for f in forms}
            res = {f: [] for f in forms}
            for r in range(a.rounds):
                for f in forms:
                    select(eng, f[0])
                    res[f].append(time_replays(gs[f][0], a.steps, gs[f][1].zero_))
            for w in wforms:
                c, s = res[(w, False)], res[(w, True)]
                mc, ms = statistics.median(c), statistics.median(s)
                line += f" weights {w}: copy {mc:.3f} ms +-{spread(c):.3f}, shared {ms:.3f} ms +-{spread(s):.3f}, {mc / ms:.3f}x |"
            print(line, flush=True)
            del gs
            torch.cuda.empty_cache()

if a.prefill:
    select(eng, "bf16")
    B, n = 4, 4
    for P in [int(p) for p in a.prefixes.split(",")]:
        ts = {}
        for rows in (B, B * n):
            x = torch.randn(rows, P, cfg.hidden, device=dev, generator=g, dtype=BF) * 0.5
            kc, vc = eng.alloc_cache(rows, P, fp8=False)
            t = []
            for r in range(a.rounds + 1):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.prefill(x, kc, vc)
                e1.record(); torch.cuda.synchronize()
                if r:                                           # round 0 warms up
                    t.append(e0.elapsed_time(e1))
            ts[rows] = t
            del x, kc, vc
            torch.cuda.empty_cache()
        print(f"prefill, sampled n-best of {n} on {B} items, prefix={P:4d}: {B * n} rows {statistics.median(ts[B * n]):.1f} ms +-{spread(ts[B * n]):.1f}, "
              f"{B} rows {statistics.median(ts[B]):.1f} ms +-{spread(ts[B]):.1f}", flush=True)
