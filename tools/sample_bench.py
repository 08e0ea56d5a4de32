#!/usr/bin/env python3
"""Sampled token step (ops.sample_rows, csrc/sample.hip) alone, against ops.argmax_rows as the yardstick: fp32 logits [B, V] at
B in {1, 8, 32}, V in {32,000 (Llama-2, rows from LDS), 128,256 (Llama-3, rows streamed from L2)}, for top-k 50 + top-p 0.9 (HF's default
with the reference's top_p), top-k off + top-p 0.9 (the full-vocabulary radix path) and top-k 1 (argmax).  Times are device events around
`--iters` back-to-back launches after a warm-up, per launch.  Then one sampled generate() against a greedy one at bench.py's decode shape
(B = 8, 256 fused AV positions, bf16 Llama-2-7B-shaped synthetic weights, 48 new tokens), per token step.
Usage: tools/sample_bench.py [--iters 200] [--no-generate]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import ops

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--no-generate", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "sample_bench needs the GPU"


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / a.iters           # us per launch


CASES = [("top-k 50 + top-p 0.9", 50, 0.9), ("top-k off + top-p 0.9", 0, 0.9), ("top-k 1", 1, 1.0)]
print(f"{'V':>7} {'B':>3}  {'argmax_rows':>12}  " + "  ".join(f"{c[0]:>22}" for c in CASES) + "   (us per launch, fp32 logits)")
for V in (32000, 128256):
    for B in (1, 8, 32):
        g = torch.Generator(device="cuda").manual_seed(V + B)
        x = torch.randn(B, V, device="cuda", generator=g) * 3
        t_am = timed(lambda: ops.argmax_rows(x))
        ts = [timed(lambda k=k, p=p: ops.sample_rows(x, 1.0, k, p, 1, 0)) for _, k, p in CASES]
        print(f"{V:>7} {B:>3}  {t_am:>12.2f}  " + "  ".join(f"{t:>22.2f}" for t in ts), flush=True)

if not a.no_generate:
    from avllm.model import ClipWhisperModel
    m = ClipWhisperModel(device="cuda:0", max_seq_len=256, precision="bf16", use_lora=False, synthetic_weights=True).eval()
    m.eos_token_id = None                                    # random weights: never stop early
    g = torch.Generator(device="cuda").manual_seed(1)
    audio = torch.randn(8, 80, 3000, device="cuda", generator=g)
    video = torch.randn(8, 125, 3, 224, 224, device="cuda", generator=g)

    def per_step(**kw):
        m.generate(audio=audio, video=video, max_new_tokens=4, **kw)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        m.generate(audio=audio, video=video, max_new_tokens=1, **kw)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        m.generate(audio=audio, video=video, max_new_tokens=48, **kw)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        return 1000.0 * ((t2 - t1) - (t1 - t0)) / 47

    for rep in range(2):                                     # alternated, twice: the spread between repeats is the noise
        gr = per_step()
        sa = per_step(do_sample=True, top_k=50, top_p=0.9, seed=1)
        print(f"generate B=8 V={m.cfg.llama.vocab} (repeat {rep}): greedy {gr:.3f} ms/step, sampled (top-k 50, top-p 0.9) {sa:.3f} ms/step, "
              f"difference {1000 * (sa - gr):+.1f} us/step", flush=True)
