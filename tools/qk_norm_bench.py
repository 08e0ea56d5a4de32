#!/usr/bin/env python3
"""What Qwen3's per-head q/k RMSNorm costs, in two measurements.

step:   the fused token step of a synthetic Qwen3-8B-shaped model (d 4096, 32 heads over 8 kv heads of 128, ffn 12288, 36 layers, vocab 151936)
        with the norms (raw q|k|v projection + one avllm_qk_norm_rope launch per layer) against the same engine with the norm pointers of its
        layer descriptors cleared (the projection rotates and writes the cache itself: the step every other model runs), alternated in one
        process, in the bf16, fp8 and fp4 weight forms.  Each step is a captured graph replayed with the position in device memory, at a
        cache position of 300.  Per cell: the median over the rounds and their spread (max - min).
kernel: avllm_qk_norm_rope (with its training saves) against the avllm_rope_tab pass it replaces, on the q|k|v buffer of a training forward
        at Qwen3-8B widths (M = 16 x 256 rows of 6144), and avllm_qk_norm_bwd; eight buffers in rotation (400 MB: past the last-level
        cache), achieved GB/s against the bytes each must move.
"""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import lib as L
from avllm import ops
from avllm.arch import LlamaCfg
from avllm.engine import LlamaEngine

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["step", "kernel"])
ap.add_argument("--batches", type=str, default="1,8,16")
ap.add_argument("--forms", type=str, default="bf16,fp8,fp4")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--layers", type=int, default=36, help="fewer than 36: a rehearsal, not a measurement")
a = ap.parse_args()
dev, BF = "cuda:0", torch.bfloat16
H, HKV, HD, D, FFN, VOCAB = 32, 8, 128, 4096, 12288, 151936
g = torch.Generator(device=dev).manual_seed(0)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for i in range(n):
        fn(i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def kernel():
    M, S, qw, nqk = 16 * 256, 256, D + 2 * HKV * HD, H + HKV
    bufs = [torch.randn(M, qw, device=dev, generator=g).to(BF) for _ in range(8)]
    wq, wk = (1 + 0.1 * torch.randn(HD, device=dev, generator=g)).to(BF), (1 + 0.1 * torch.randn(HD, device=dev, generator=g)).to(BF)
    tab = ops.rope_table(S, HD, 0, 1e6)
    pre, rstd = ops.qk_norm_rope_(bufs[0], S, H, HKV, HD, wq, wk, 1e-6, tab, save=True)
    lib, st = L.load(), L.stream_ptr()
    qk = M * nqk * HD * 2                              # bytes of the q and k slices
    runs = {
        "rope_tab (replaced)": (lambda i: ops.rope_tab_(bufs[i % 8], S, nqk, HD, tab), 2 * qk),
        "qk_norm_rope, no saves": (lambda i: ops.qk_norm_rope_(bufs[i % 8], S, H, HKV, HD, wq, wk, 1e-6, tab), 2 * qk),
        "qk_norm_rope + saves": (lambda i: L.check(lib.avllm_qk_norm_rope(L.ptr(bufs[i % 8]), qw, M, S, H, HKV, HD, L.ptr(wq), L.ptr(wk), 1e-6, L.ptr(tab),
                                                                        L.ptr(pre), L.ptr(rstd), None, None, 0, 0, None, L.BF16, st)), 3 * qk + M * nqk * 4),
        "qk_norm_bwd": (lambda i: ops.qk_norm_bwd_(bufs[i % 8], H, HKV, HD, wq, wk, pre, rstd), 3 * qk + M * nqk * 4),
    }
    print(f"M = {M} rows of {qw} bf16 (q|k = {nqk} heads of {HD}); extra activation memory per layer with the norms: "
          f"{(qk + M * nqk * 4) / 1e6:.1f} MB (pre-norm q|k {qk / 1e6:.1f} MB + rstd {M * nqk * 4 / 1e6:.2f} MB)", flush=True)
    for name, (fn, nbytes) in runs.items():
        timed(fn, 16)
        ts = [timed(fn, 200) for _ in range(a.rounds)]
        med = statistics.median(ts)
        print(f"{name:24s} {med * 1e3:7.1f} us +-{(max(ts) - min(ts)) * 1e3:.1f}  {nbytes / 1e6:.1f} MB moved  {nbytes / med / 1e6:.0f} GB/s", flush=True)


def step():
    forms = a.forms.split(",")
    cfg = LlamaCfg(D, H, a.layers, FFN, VOCAB, 1e-6, 1e6, HKV, (), False, False, True)
    dkv = HKV * HD
    w = lambda o, k: torch.randn(o, k, device=dev, generator=g, dtype=BF) * k ** -0.5
    one = lambda n: torch.ones(n, device=dev, dtype=BF)
    sd = {"model.embed_tokens.weight": w(VOCAB, D), "model.norm.weight": one(D), "lm_head.weight": w(VOCAB, D)}
    for i in range(cfg.layers):
        p = f"model.layers.{i}."
        for nm, (o, k) in {"self_attn.q_proj": (D, D), "self_attn.k_proj": (dkv, D), "self_attn.v_proj": (dkv, D), "self_attn.o_proj": (D, D),
                           "mlp.gate_proj": (FFN, D), "mlp.up_proj": (FFN, D), "mlp.down_proj": (D, FFN)}.items():
            sd[p + nm + ".weight"] = w(o, k)
        for nm in ("input_layernorm", "post_attention_layernorm"):
            sd[p + nm + ".weight"] = one(D)
        for nm in ("q_norm", "k_norm"):
            sd[p + f"self_attn.{nm}.weight"] = (1 + 0.1 * torch.randn(HD, device=dev, generator=g)).to(BF)
    eng = LlamaEngine(sd, cfg, None, None, dtype=BF, device=dev, training=False, decode_fp8=True)
    if "fp4" in forms:
        for i in range(cfg.layers):
            p = f"model.layers.{i}."
            cat = lambda *ks: torch.cat([sd[p + k + ".weight"] for k in ks], 0)
            eng._fp4_images(eng.layers[i], cat("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), sd[p + "self_attn.o_proj.weight"],
                            cat("mlp.gate_proj", "mlp.up_proj"), sd[p + "mlp.down_proj.weight"])
    del sd
    norms = [(ly.q_norm_w, ly.k_norm_w) for ly in eng.layers]
    torch.cuda.synchronize()

    def select(form, qk):
        eng.desc.decode_fp8, eng.desc.decode_fp4 = int(form == "fp8"), int(form == "fp4")
        for ly, (q, k) in zip(eng.layers, norms):
            ly.q_norm_w, ly.k_norm_w = (q, k) if qk else (None, None)

    def graph(B, form, qk):
        select(form, qk)
        assert eng.decode_is_fused(B) and eng.decode_streams_fp8(B) == (form == "fp8") and eng.decode_streams_fp4(B) == (form == "fp4")
        kc, vc = eng.alloc_cache(B, 320 + a.steps + 8)
        ids = torch.randint(0, VOCAB, (B,), device=dev, generator=g)
        pd = torch.zeros(1, device=dev, dtype=torch.int32)
        out = torch.empty(B, VOCAB, device=dev, dtype=torch.float32)
        eng.decode_step(ids, 300, kc, vc, pos_dev=pd, logits=out)
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
        return timed(lambda i: gr.replay(), a.steps)

    print(f"Qwen3-8B shapes, {cfg.layers} layers, token step at cache position 300: with the head norms / without (ms, median of {a.rounds} "
          f"rounds of {a.steps} steps, +- spread)", flush=True)
    for B in [int(b) for b in a.batches.split(",")]:
        for f in forms:
            gs = {qk: graph(B, f, qk) for qk in (True, False)}
            res = {True: [], False: []}
            for r in range(a.rounds):
                for qk in (True, False):
                    res[qk].append(time_graph(*gs[qk][:2]))
            m1, m0 = statistics.median(res[True]), statistics.median(res[False])
            print(f"B={B:2d} {f:4s}  with {m1:.3f} +-{max(res[True]) - min(res[True]):.3f}   without {m0:.3f} +-{max(res[False]) - min(res[False]):.3f}   "
                  f"extra {1e3 * (m1 - m0):6.1f} us = {1e3 * (m1 - m0) / cfg.layers:.2f} us per layer ({100 * (m1 / m0 - 1):.2f} %)", flush=True)
            del gs
            torch.cuda.empty_cache()


kernel() if a.what == "kernel" else step()
