#!/usr/bin/env python3
"""Token-step time of a model whose adapters were merged (LlamaEngine.merge_lora) against the same model with its adapters separate and
against a model built without adapters, at Llama-2-7B shapes with synthetic weights: three engines in one process (rank-16 adapters on q, k, v,
o; each engine holds the bf16 matrices and their fp8 and fp4 token-step images, the descriptor's decode_fp8 / decode_fp4 flags select the form
a step streams), alternated round by round.  Each step is a captured hipGraph replayed with the position in device memory at a cache position
of 300, as tools/decode_step_bench.py measures it.  Per leg: the median over the rounds and their spread (max - min).  The expectation checked
and printed: the merged leg equals the no-adapter leg of the same run within the larger of the two spreads (the same kernels on the same number
of bytes).  Also timed, once: merge_lora() itself (wall clock, images included), its merge launches alone, and a plain device copy of the bytes
those launches read and write."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import lib as L
from avllm import ops
from avllm.arch import LlamaCfg, LoraCfg
from avllm.engine import LORA_TARGETS, LlamaEngine

ap = argparse.ArgumentParser()
ap.add_argument("--batches", type=str, default="1,8,16")
ap.add_argument("--forms", type=str, default="bf16,fp8,fp4")
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--layers", type=int, default=0, help="fewer layers than the model's 32: a rehearsal, not a measurement")
a = ap.parse_args()
forms = a.forms.split(",")
assert forms and all(f in ("bf16", "fp8", "fp4") for f in forms), forms
dev, BF = "cuda:0", torch.bfloat16
cfg = LlamaCfg(4096, 32, a.layers or 32, 11008, 32000)
g = torch.Generator(device=dev).manual_seed(0)


def w(o, k):
    return (torch.randn(o, k, device=dev, generator=g, dtype=BF) * k ** -0.5)


sd = {"model.embed_tokens.weight": w(cfg.vocab, cfg.hidden), "model.norm.weight": torch.ones(cfg.hidden, device=dev, dtype=BF),
      "lm_head.weight": w(cfg.vocab, cfg.hidden)}
for i in range(cfg.layers):
    p = f"model.layers.{i}."
    for nm, (o, k) in {"self_attn.q_proj": (cfg.hidden, cfg.hidden), "self_attn.k_proj": (cfg.hidden, cfg.hidden), "self_attn.v_proj": (cfg.hidden, cfg.hidden),
                       "self_attn.o_proj": (cfg.hidden, cfg.hidden), "mlp.gate_proj": (cfg.ffn, cfg.hidden), "mlp.up_proj": (cfg.ffn, cfg.hidden),
                       "mlp.down_proj": (cfg.hidden, cfg.ffn)}.items():
        sd[p + nm + ".weight"] = w(o, k)
    sd[p + "input_layernorm.weight"] = torch.ones(cfg.hidden, device=dev, dtype=BF)
    sd[p + "post_attention_layernorm.weight"] = torch.ones(cfg.hidden, device=dev, dtype=BF)
lora_draw = None


def engine(lora):
    """An engine with all three weight forms: built with the fp8 token-step images, the fp4 ones added beside them (an engine built with
    decode_fp4=True holds them instead) and registered where merge_lora() looks for the images it has to rebuild."""
    global lora_draw
    eng = LlamaEngine(sd, cfg, LoraCfg(a.rank, 2.0 * a.rank) if lora else None, None, dtype=BF, device=dev, training=False, decode_fp8=True)
    if "fp4" in forms:
        for i in range(cfg.layers):
            k = lambda nm: eng.llm_w[f"model.layers.{i}.{nm}.weight"]
            img = eng._fp4_images(eng.layers[i], eng.llm_w[i, "qkv"], k("self_attn.o_proj"), eng.llm_w[i, "gu"], k("mlp.down_proj"))
            eng.img4[i, "qkv"], eng.img4[i, "o"] = img["qkv"], img["o"]
    if lora:
        if lora_draw is None:
            lora_draw = torch.randn(eng.lora_p.shape, device=dev, generator=g) * 0.01
        eng.lora_p.copy_(lora_draw)                  # the same adapters in both engines that have them
        eng.pack_lora()
    return eng


legs = {"adapters": engine(True), "merged": engine(True), "none": engine(False)}
torch.cuda.synchronize()

# ---- the merge itself, once: the merge launches alone on scratch copies, a device copy of the same bytes, then merge_lora() as a whole
em = legs["merged"]
views = em.lora_views()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


scratch = [(em.llm_w[i, "qkv"].clone(), em.llm_w[f"model.layers.{i}.self_attn.o_proj.weight"].clone()) for i in range(cfg.layers)]
dst = [(q.clone(), o.clone()) for q, o in scratch]
nbytes_merge = 2 * sum(q.numel() * 2 + o.numel() * 2 for q, o in scratch)      # read once, written once


def merge_launches():
    for i, (wqkv, wo) in enumerate(scratch):
        for j, nm in enumerate(LORA_TARGETS):
            lo, hi = em._qkv_rows()[j] if j < 3 else (0, 0)
            ops.lora_merge_(wo if j == 3 else wqkv[lo:hi], views[f"layers.{i}.{nm}.lora_A"], views[f"layers.{i}.{nm}.lora_B"], em.lcfg.scale)


def copies():
    for (q, o), (dq, do) in zip(scratch, dst):
        dq.copy_(q); do.copy_(o)


merge_launches(); copies()                           # warm-up: code objects loaded, clocks up
t_launch = [timed(merge_launches) for _ in range(a.rounds)]
t_copy = [timed(copies) for _ in range(a.rounds)]
del scratch, dst
torch.cuda.synchronize()
t0 = time.perf_counter()
em.merge_lora()
torch.cuda.synchronize()
t_merge = (time.perf_counter() - t0) * 1e3
med = statistics.median
print(f"llama2-7b, {cfg.layers} layers, rank {a.rank}: merge launches alone ({4 * cfg.layers} launches, {nbytes_merge / 1e9:.2f} GB read + written) "
      f"{med(t_launch):.2f} ms +-{max(t_launch) - min(t_launch):.2f} ({nbytes_merge / med(t_launch) / 1e9:.2f} TB/s); device copy of the same bytes "
      f"{med(t_copy):.2f} ms +-{max(t_copy) - min(t_copy):.2f} ({nbytes_merge / med(t_copy) / 1e9:.2f} TB/s); merge_lora() as a whole, wall clock, once, "
      f"with {'the fp8 and fp4' if 'fp4' in forms else 'the fp8'} images of wqkv and wo rebuilt: {t_merge:.1f} ms", flush=True)


def select(eng, form):
    eng.desc.decode_fp8, eng.desc.decode_fp4 = int(form == "fp8"), int(form == "fp4")


def graph(eng, B, form):
    select(eng, form)
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


assert all(not ly.lora[j].A_pad for ly in legs["merged"].layers for j in range(4)) and all(ly.lora[0].A_pad for ly in legs["adapters"].layers)
for form in forms:
    for B in [int(b) for b in a.batches.split(",")]:
        gs = {n: graph(e, B, form) for n, e in legs.items()}
        res = {n: [] for n in legs}
        for r in range(a.rounds):
            for n in legs:
                res[n].append(time_graph(*gs[n][:2]))
        m = {n: med(res[n]) for n in legs}
        sp = {n: max(res[n]) - min(res[n]) for n in legs}
        diff, allow = abs(m["merged"] - m["none"]), max(sp["merged"], sp["none"])
        print(f"{form} B={B:2d}  " + "  ".join(f"{n} {m[n]:.3f} ms +-{sp[n]:.3f}" for n in legs) +
              f"  adapters/merged {m['adapters'] / m['merged']:.3f}x  |merged - none| {diff:.3f} ms vs spread {allow:.3f}: "
              f"{'equal within the spread' if diff <= allow else 'NOT equal within the spread'}"
              "  rounds " + " ".join(f"{n} {[round(x, 3) for x in res[n]]}" for n in legs), flush=True)
        del gs
        torch.cuda.empty_cache()
