#!/usr/bin/env python3
"""Time of the logits-processor launch (csrc/logits_process.hip) with the sequence-bias / bad-words / suppress tables, beside the launch
of the three older processors alone: ops.logits_process on f32 scores [rows, V] with a 64-token history, rows in {8, 32}, V in {32000,
151936}, 0 / 64 / 1024 sequences of 1 to 4 tokens (half of them on the rows' own tails, so they apply), and a suppress list of all but 100
ids.  Each form is timed as --iters back-to-back launches between two events, queued behind two large matrix products so that the host has
issued all of them before the first one starts (device time, not the host's issue rate); the forms are alternated in one process and the
median of --rounds rounds is reported (rounds listed).  The scores are processed in place again and again: their values drift, the work does not."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))

import torch  # noqa: E402
from avllm import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--iters", type=int, default=200); ap.add_argument("--hist", type=int, default=64)
a = ap.parse_args()
OLD = dict(repetition_penalty=1.2, no_repeat_ngram_size=3)


def sequences(n, hist, V, g):
    out = {}
    rnd = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g))  # noqa: E731
    while len(out) < n:
        L = rnd(1, 5)
        pre = hist[rnd(0, hist.shape[0]), hist.shape[1] - (L - 1):].tolist() if L > 1 else []
        if pre and rnd(0, 2):
            pre[0] = rnd(0, V)
        out[tuple(pre) + (rnd(0, V),)] = 0.5
    return out


def forms(rows, V):
    g = torch.Generator().manual_seed(rows + V)
    hist = torch.randint(0, V, (rows, a.hist), generator=g)
    allow = set(range(1000, 1100))
    sup = [t for t in range(V) if t not in allow]
    tb = {n: ops.logits_bias_tables(sequences(n, hist, V, g), [list(q) for q in sequences(n, hist, V, g)], vocab=V) for n in (64, 1024)}
    st = ops.logits_bias_tables(suppress_tokens=sup, begin_suppress_tokens=[1, 2], vocab=V)
    h = hist.cuda()
    return [("penalty 1.2 + 3-gram ban (the older launch)", h, OLD, {}),
            ("  + 64 bias + 64 bad sequences", h, OLD, tb[64]),
            ("  + 1024 bias + 1024 bad sequences", h, OLD, tb[1024]),
            ("  + suppress V-100 ids", h, OLD, st),
            ("  + 1024 + 1024 sequences + suppress V-100 ids", h, OLD, dict(tb[1024], **st)),
            ("suppress V-100 ids alone (no history)", None, {}, st),
            ("1024 bias sequences alone", h, {}, {"sequence_bias": tb[1024]["sequence_bias"]})]


BIG = torch.randn(8192, 8192, device="cuda")


def launch_us(scores, h, kw, tables):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.mm(BIG, BIG); torch.mm(BIG, BIG)                   # keeps the device busy while the launches below are issued
    e0.record()
    for _ in range(a.iters):
        ops.logits_process(scores, h, a.hist, **kw, **tables)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters


print(f"ops.logits_process, f32 scores, {a.hist}-token history: us per launch, median of {a.rounds} rounds of {a.iters} launches")
for rows in (8, 32):
    for V in (32000, 151936):
        scores = torch.randn(rows, V, device="cuda")
        legs = forms(rows, V)
        for _, h, kw, tables in legs:
            launch_us(scores, h, kw, tables)
        times = {name: [] for name, *_ in legs}
        for _ in range(a.rounds):
            for name, h, kw, tables in legs:
                times[name].append(launch_us(scores, h, kw, tables))
        print(f"rows = {rows}, V = {V}")
        for name, *_ in legs:
            t = times[name]
            print(f"  {name:48s} {statistics.median(t):8.2f} us   rounds {[round(x, 2) for x in t]}")
