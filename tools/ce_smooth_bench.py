#!/usr/bin/env python3
"""Times the cross-entropy kernels with label smoothing and z-loss (avllm_ce_smooth_fwd / _bwd at eps = 0.1, z = 1e-4) against the plain pair
(avllm_ce_fwd / avllm_ce_bwd) in one process, on [16 * 256, 32000] (Llama-2) and [16 * 256, 152064] (Qwen) bf16 logits, every row scored.
Both pairs read the logits once per launch and the backward writes them once, in place as the engine does (the values drift from launch to
launch; the kernels' time does not depend on them), so the expectation from the byte count is parity.  Five rounds, the legs alternated within a
round, the median per leg and the round-to-round spread (min .. max); device events around 20 launches per leg.  No ratio is asserted: the
yardstick is the existing kernel in the same run."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import lib as L

EPS, Z = 0.1, 1e-4


def timed(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000


dev, bf = "cuda", torch.bfloat16
B, T = 16, 256
lib = L.load()
print(f"bf16 logits [{B} * {T}, V], every row but a sequence's last scored; microseconds per launch, median of 5 rounds (min .. max)")
for V in (32000, 152064):
    g = torch.Generator(device=dev).manual_seed(0)
    logits = torch.randn(B, T, V, device=dev, generator=g).to(bf)
    labels = torch.randint(0, V, (B, T), device=dev, generator=g)
    row_lse = torch.empty(B * T, device=dev, dtype=torch.float32)
    acc = torch.zeros(2, device=dev, dtype=torch.float32)
    terms = torch.zeros(3, device=dev, dtype=torch.float32)
    one = torch.ones(1, device=dev, dtype=torch.float32)
    p = lambda t: L.ptr(t)
    st = L.stream_ptr()
    legs = [
        ("ce_fwd", lambda: L.check(lib.avllm_ce_fwd(p(logits), V, p(labels), B, T, V, p(row_lse), p(acc), p(acc) + 4, 1, st))),
        ("ce_smooth_fwd", lambda: L.check(lib.avllm_ce_smooth_fwd(p(logits), V, p(labels), B, T, V, EPS, Z, p(row_lse), p(acc), p(acc) + 4, p(terms), 1, st))),
        ("ce_smooth_fwd, terms = NULL", lambda: L.check(lib.avllm_ce_smooth_fwd(p(logits), V, p(labels), B, T, V, EPS, Z, p(row_lse), p(acc), p(acc) + 4, None, 1, st))),
        ("ce_bwd", lambda: L.check(lib.avllm_ce_bwd(p(logits), V, p(labels), p(row_lse), p(one), 1.0, p(logits), B, T, V, 1, st))),
        ("ce_smooth_bwd", lambda: L.check(lib.avllm_ce_smooth_bwd(p(logits), V, p(labels), p(row_lse), p(one), 1.0, EPS, Z, p(logits), B, T, V, 1, st))),
    ]
    rounds = [[timed(fn) for _, fn in legs] for _ in range(5)]
    med = []
    for i, (name, _) in enumerate(legs):
        ts = [r[i] for r in rounds]
        med.append(statistics.median(ts))
        gbs = (B * T * V * 2 * (2 if "bwd" in name else 1)) / (med[-1] * 1e-6) / 1e9
        print(f"V = {V:<7d} {name:<28s} {med[-1]:8.1f}   ({min(ts):.1f} .. {max(ts):.1f})   {gbs:7.0f} GB/s")
    print(f"V = {V:<7d} smooth / plain: fwd {med[1] / med[0]:.3f}, bwd {med[4] / med[3]:.3f}")
    del logits
