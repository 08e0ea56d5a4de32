#!/usr/bin/env python3
"""Beam-search device ops (csrc/beam.hip) and beam-search generate().
Per launch (device events around `--iters` back-to-back launches after a warm-up):
  * ops.beam_topk at B x nb in {4x4, 8x4} (k = 2*nb), V in {32,000, 128,256}, fp32 logits, against ops.argmax_rows on the same rows;
  * ops.kv_gather_rows at bench.py's decode shape (Llama-2-7B: 32 layers, dkv 4096, bf16, S = 256, 16 rows), in place, every row taking
    another row's history (the kernel's worst case: no identity rows to skip): the suffix reorder [S, S + step) at steps 16 and 48, against a
    full-prefix reorder [0, S + step) (what HF's _reorder_cache moves) and torch's index_select of the full cache.  Bytes = read + write.
Per token step: generate(num_beams=4) against greedy on B and on 4*B items (the same row count) at bench.py's decode shape (256 fused AV positions, bf16 Llama-2-7B-shaped synthetic
weights, 48 new tokens, no EOS), at B = 4 (16 rows: fused step) and B = 8 (32 rows: general step).
Usage: tools/beam_bench.py [--iters 200] [--no-generate]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import ops

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--no-generate", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "beam_bench needs the GPU"
HBM_PEAK = 8.0e12


def timed(fn, iters=None):
    iters = iters or a.iters
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / iters           # us per launch


print(f"{'V':>7} {'B x nb':>7}  {'argmax_rows':>12}  {'beam_topk (k=2nb)':>18}  {'ratio':>6}   (us per launch, fp32 logits)")
for V in (32000, 128256):
    for B, nb in ((4, 4), (8, 4)):
        g = torch.Generator(device="cuda").manual_seed(V + B)
        x = torch.randn(B * nb, V, device="cuda", generator=g) * 3
        sc = -torch.rand(B * nb, device="cuda", generator=g)
        t_am = timed(lambda: ops.argmax_rows(x))
        t_bt = timed(lambda: ops.beam_topk(x, sc, nb, 2 * nb))
        print(f"{V:>7} {f'{B}x{nb}':>7}  {t_am:>12.2f}  {t_bt:>18.2f}  {t_bt / t_am:>6.2f}", flush=True)

layers, R, S, dkv, N = 32, 16, 256, 4096, 64
kc = torch.randn(layers, R, S + N, dkv, device="cuda", dtype=torch.bfloat16)
vc = torch.randn_like(kc)
parent = ((torch.arange(R, device="cuda") // 4) * 4 + (torch.arange(R, device="cuda") + 1) % 4).to(torch.int32)   # cyclic within each item
print(f"kv_gather_rows, in place, {layers} layers x {R} rows x dkv {dkv} bf16, S = {S}, every row from another row (read + write bytes):")
for step in (16, 48):
    for name, t0, t1 in (("suffix [S, S+step)", S, S + step), ("full [0, S+step)", 0, S + step)):
        nbytes = 2 * 2 * layers * R * (t1 - t0) * dkv * 2
        t = timed(lambda: ops.kv_gather_rows(kc, vc, kc, vc, parent, t0, t1), iters=50)
        print(f"  step {step:>2} {name:>20}: {t:9.1f} us  {nbytes / 1e6:8.1f} MB  {nbytes / t / 1e6:6.2f} TB/s ({100 * nbytes / t / 1e6 / (HBM_PEAK / 1e12):.0f} % of 8 TB/s)",
              flush=True)
    pl = parent.long()
    full = lambda: (kc[:, :, :S + step].index_select(1, pl), vc[:, :, :S + step].index_select(1, pl))  # noqa: E731
    t = timed(full, iters=20)
    nbytes = 2 * 2 * layers * R * (S + step) * dkv * 2
    print(f"  step {step:>2} {'torch index_select':>20}: {t:9.1f} us  {nbytes / 1e6:8.1f} MB  {nbytes / t / 1e6:6.2f} TB/s  (HF's full reorder, out of place)",
          flush=True)
del kc, vc

if not a.no_generate:
    from avllm.model import ClipWhisperModel
    m = ClipWhisperModel(device="cuda:0", max_seq_len=256, precision="bf16", use_lora=False, synthetic_weights=True).eval()
    m.eos_token_id = None                                    # random weights: never stop early

    def per_step(audio, video, **kw):
        m.generate(audio=audio, video=video, max_new_tokens=4, **kw)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        m.generate(audio=audio, video=video, max_new_tokens=1, **kw)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        m.generate(audio=audio, video=video, max_new_tokens=48, **kw)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        return 1000.0 * ((t2 - t1) - (t1 - t0)) / 47

    for B in (4, 8):
        g = torch.Generator(device="cuda").manual_seed(1)
        audio = torch.randn(4 * B, 80, 3000, device="cuda", generator=g)
        video = torch.randn(4 * B, 125, 3, 224, 224, device="cuda", generator=g)
        path = "fused" if m.llm_engine.decode_is_fused(4 * B) else "general"
        for rep in range(2):                                 # alternated, twice: the spread between repeats is the noise
            gr = per_step(audio[:B], video[:B])
            gr4 = per_step(audio, video)                     # greedy on as many rows as the beams: the same token step
            bm = per_step(audio[:B], video[:B], num_beams=4)
            print(f"generate B={B} V={m.cfg.llama.vocab} (repeat {rep}): greedy {B} rows {gr:.3f} ms/step, greedy {4 * B} rows {gr4:.3f} ms/step, "
                  f"num_beams=4 ({4 * B} rows, {path} step) {bm:.3f} ms/step: beam minus greedy on {4 * B} rows {1000 * (bm - gr4):+.0f} us/step",
                  flush=True)
        del audio, video
        torch.cuda.empty_cache()
