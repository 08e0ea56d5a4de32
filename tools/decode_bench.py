#!/usr/bin/env python3
"""Greedy-decode throughput (ClipWhisperModel.generate): prefill on L=256 fused AV frames + N single-token steps with a KV cache.
HBM roofline for a step = bf16 weight bytes (6.74 G params x 2 B = 13.5 GB) / 6.29 TB/s measured copy bandwidth."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm.model import ClipWhisperModel

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8); ap.add_argument("--new", type=int, default=64); ap.add_argument("--frames", type=int, default=125)
ap.add_argument("--decode_weights", choices=["bf16", "fp8", "fp4"], default="bf16")
a = ap.parse_args()
m = ClipWhisperModel(device="cuda:0", max_seq_len=256, precision="bf16", use_lora=False, synthetic_weights=True, decode_weights=a.decode_weights).eval()
m.eos_token_id = None                                    # random weights: never stop early
g = torch.Generator(device="cuda").manual_seed(1)
audio = torch.randn(a.batch, 80, 3000, device="cuda", generator=g)
video = torch.randn(a.batch, a.frames, 3, 224, 224, device="cuda", generator=g)
m.generate(audio=audio, video=video, max_new_tokens=4)
torch.cuda.synchronize(); t0 = time.perf_counter()
ids = m.generate(audio=audio, video=video, max_new_tokens=1)
torch.cuda.synchronize(); t1 = time.perf_counter()
ids = m.generate(audio=audio, video=video, max_new_tokens=a.new)
torch.cuda.synchronize(); t2 = time.perf_counter()
step = ((t2 - t1) - (t1 - t0)) / (a.new - 1)
wbytes = sum(p.numel() * p.element_size() for p in m.llm_engine.keep) / 2    # engine holds weight + transposed image when training=True
print(f"B={a.batch}: encode+prefill {1000*(t1-t0):.1f} ms, {1000*step:.3f} ms/step, {a.batch/step:.1f} tok/s, "
      f"weights streamed per step ~13.5 GB -> {13.5e9/step/1e12:.2f} TB/s ({13.5e9/step/6.29e12*100:.0f}% of measured HBM copy rate)")
