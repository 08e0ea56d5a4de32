#!/usr/bin/env python3
"""Times the per-clip modality kernels against the kernels they stand beside, in one process: avllm_fuse_pool_rows against avllm_fuse_pool,
avllm_fuse_pool_rows_bwd against avllm_fuse_pool_bwd, and the avllm_modality_draw launch alone, at [16, 256, 4096] bf16 with Ta = 256,
Tv = 125, P = 32 (the bench shape's fusion).  The rows kernels move the same bytes plus the 16 mode words; the modes are mixed (a third of
the clips each), so the rows legs read FEWER input rows than the two-input legs -- the all-zero modes are timed too, which read the same.
Five rounds, the legs alternated within a round, the median per leg and the round-to-round spread (min .. max); device events around 50
launches per leg.  No ratio is asserted: the yardstick is the existing kernel in the same run."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import ops


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000


dev, bf = "cuda", torch.bfloat16
B, S, D, Ta, Tv, P, FS = 16, 256, 4096, 256, 125, 32, 0.5
Lc = S
g = torch.Generator(device=dev).manual_seed(0)
rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)
a, v, pe, dx = rn(B, Ta, D), rn(B, Tv, D), rn(B, P, D), rn(B, S, D)
da, dv = torch.empty(B, Ta, D, device=dev, dtype=bf), torch.empty(B, Tv, D, device=dev, dtype=bf)
mixed = torch.tensor([b % 3 for b in range(B)], dtype=torch.int32, device=dev)
zeros = torch.zeros(B, dtype=torch.int32, device=dev)
seed_word = torch.tensor([12345], dtype=torch.int32, device=dev)
drawn = torch.empty(B, dtype=torch.int32, device=dev)

legs = [
    ("fuse_pool            (a, v)", lambda: ops.fuse_pool(a, v, pe, Lc, S, FS, D, B)),
    ("fuse_pool_rows       modes all 0", lambda: ops.fuse_pool_rows(a, v, pe, zeros, Lc, S, FS, D, B)),
    ("fuse_pool_rows       modes 0,1,2,...", lambda: ops.fuse_pool_rows(a, v, pe, mixed, Lc, S, FS, D, B)),
    ("fuse_pool_bwd        -> da, dv", lambda: ops.fuse_pool_bwd(dx, Ta, Tv, P, Lc, FS, da=da, dv=dv)),
    ("fuse_pool_rows_bwd   modes all 0", lambda: ops.fuse_pool_rows_bwd(dx, zeros, Ta, Tv, P, Lc, FS, da=da, dv=dv)),
    ("fuse_pool_rows_bwd   modes 0,1,2,...", lambda: ops.fuse_pool_rows_bwd(dx, mixed, Ta, Tv, P, Lc, FS, da=da, dv=dv)),
    ("modality_draw        B = 16, device seed", lambda: ops.modality_draw(B, 0.25, 0.25, seed_dev=seed_word, out=drawn)),
]
# the forward legs allocate their output (torch's caching allocator: no device call after the first round), as the model's call does
rounds = [[timed(fn) for _, fn in legs] for _ in range(5)]
print(f"[{B}, {S}, {D}] bf16, Ta = {Ta}, Tv = {Tv}, P = {P}; microseconds per launch, median of 5 rounds (min .. max)")
for i, (name, _) in enumerate(legs):
    ts = [r[i] for r in rounds]
    print(f"{name:<42s} {statistics.median(ts):8.1f}   ({min(ts):.1f} .. {max(ts):.1f})")
