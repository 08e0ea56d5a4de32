#!/usr/bin/env python3
"""Token scores (ops.row_scores, csrc/token_score.hip) alone: fp32 logits [16, V] at V in {32,000, 128,256, 151,936}, logprob + entropy and
logprob alone, with ops.argmax_rows on the same rows as the yardstick.  The kernel reads each row once, so the rate is rows * V * 4 bytes
over the launch time; with one workgroup per row, 16 rows occupy 16 of the CUs and the figure is the rate of those, not of the chip.  Times
are device events around `--iters` back-to-back launches after a warm-up, per launch (the rows stay in the caches between launches, as
they do after the lm_head GEMM of a token step).  Then one greedy generate() with and without return_token_scores at bench.py's decode
shape (B = 8, 256 fused AV positions, bf16 Llama-2-7B-shaped synthetic weights, 48 new tokens), per token step, alternated.
Usage: tools/token_score_bench.py [--iters 200] [--no-generate]"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import ops

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--no-generate", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "token_score_bench needs the GPU"


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


B = 16
print(f"{'V':>7} {'B':>3}  {'argmax_rows':>12}  {'row_scores':>12}  {'+ entropy':>12}  {'GB/s (+ entropy)':>17}  {'log-prob rows':>14}   (us per launch, fp32 logits)")
for V in (32000, 128256, 151936):
    g = torch.Generator(device="cuda").manual_seed(V)
    x = torch.randn(B, V, device="cuda", generator=g) * 3
    tok = torch.randint(0, V, (B,), device="cuda", generator=g)
    lsm = torch.log_softmax(x, 1)
    for rep in range(2):                                     # twice: the spread between repeats is the noise
        t_am = timed(lambda: ops.argmax_rows(x))
        t_lp = timed(lambda: ops.row_scores(x, tok))
        t_en = timed(lambda: ops.row_scores(x, tok, entropy=True))
        t_ls = timed(lambda: ops.row_scores(lsm, tok, entropy=True, logprobs=True))
        print(f"{V:>7} {B:>3}  {t_am:>12.2f}  {t_lp:>12.2f}  {t_en:>12.2f}  {B * V * 4 / t_en / 1e3:>17.1f}  {t_ls:>14.2f}", flush=True)

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

    for rep in range(3):                                     # alternated: the spread between repeats is the noise
        plain = per_step()
        scored = per_step(return_token_scores=True)
        print(f"generate B=8 V={m.cfg.llama.vocab} (repeat {rep}): greedy {plain:.3f} ms/step, with return_token_scores {scored:.3f} ms/step, "
              f"difference {1000 * (scored - plain):+.1f} us/step ({100 * (scored - plain) / plain:+.2f} %)", flush=True)
