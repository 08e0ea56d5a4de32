#!/usr/bin/env python3
"""Cost of generate()'s logits processors per token: greedy ClipWhisperModel.generate at Llama-2-7B shapes (synthetic weights), time per
token = (t(N new tokens) - t(1 new token)) / (N - 1), for
  * knobs off on another build of the package (--parent-tree: a checkout of the parent commit with its library built), when given;
  * knobs off on this tree;
  * repetition_penalty=1.2, no_repeat_ngram_size=3 on this tree;
alternated in one process, minimum of --rounds rounds (rounds listed)."""
import argparse, importlib, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8); ap.add_argument("--new", type=int, default=100); ap.add_argument("--frames", type=int, default=125)
ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--parent-tree", default=None)
a = ap.parse_args()


def package(root):
    """avllm.model.ClipWhisperModel of the tree at `root`, imported apart from any avllm already loaded (each binds its own libavllm.so)."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "avllm" or k.startswith("avllm.")}
    sys.path.insert(0, os.path.join(root, "audio-visual-llm_amd"))
    try:
        cls = importlib.import_module("avllm.model").ClipWhisperModel
    finally:
        sys.path.pop(0)
        for k in [k for k in sys.modules if k == "avllm" or k.startswith("avllm.")]:
            del sys.modules[k]
        sys.modules.update(saved)
    return cls


import torch  # noqa: E402

g = torch.Generator(device="cuda").manual_seed(1)
audio = torch.randn(a.batch, 80, 3000, device="cuda", generator=g)
video = torch.randn(a.batch, a.frames, 3, 224, 224, device="cuda", generator=g)


def model(root):
    m = package(root)(device="cuda:0", max_seq_len=256, precision="bf16", use_lora=False, synthetic_weights=True).eval()
    m.eos_token_id = None                                    # random weights: never stop early
    return m


def per_token(m, **kw):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    m.generate(audio=audio, video=video, max_new_tokens=1, **kw)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    m.generate(audio=audio, video=video, max_new_tokens=a.new, **kw)
    torch.cuda.synchronize(); t2 = time.perf_counter()
    return ((t2 - t1) - (t1 - t0)) / (a.new - 1) * 1e6


ON = dict(repetition_penalty=1.2, no_repeat_ngram_size=3)
legs = []
if a.parent_tree:
    legs.append(("parent, knobs off", model(a.parent_tree), {}))
here = model(ROOT)
legs += [("this tree, knobs off", here, {}), ("this tree, penalty 1.2 + 3-gram ban", here, ON)]
for _, m, kw in legs:
    m.generate(audio=audio, video=video, max_new_tokens=4, **kw)
times = {name: [] for name, _, _ in legs}
for _ in range(a.rounds):
    for name, m, kw in legs:
        times[name].append(per_token(m, **kw))
print(f"greedy generate, B = {a.batch}, {a.new} new tokens, Llama-2-7B shapes, bf16: us per token, min of {a.rounds} rounds")
for name, _, _ in legs:
    t = times[name]
    print(f"{name:38s} {min(t):9.1f} us   rounds {[round(x, 1) for x in t]}   spread {max(t) - min(t):.1f} us")
base = min(times["this tree, knobs off"])
print(f"knobs on - knobs off = {min(times['this tree, penalty 1.2 + 3-gram ban']) - base:+.1f} us per token")
if a.parent_tree:
    print(f"this tree - parent (knobs off) = {base - min(times['parent, knobs off']):+.1f} us per token")
