#!/usr/bin/env python3
"""Times the acoustic augmentation kernels (csrc/augment.hip) against what stands beside them, in one process: avllm_wave_add_noise (both
launches: energies, mix) at 16 x 480000 samples, out of place and in place, against a device-to-device copy of the same bytes and against
avllm_logmel of the same batch (the step it precedes); avllm_spec_augment at [16, 80, 3000] and [16, 128, 3000] against a device-to-device
copy of the tensor (the masking writes only the masked cells, so the copy is an upper yardstick, not a peer).  Five rounds, the legs
alternated within a round, the median per leg and the round-to-round spread (min .. max); device events around 20 launches per leg.  No ratio
is asserted."""
import os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm.preprocess import AudioAugment, NoiseBank, WhisperLogMel


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


dev = "cuda"
B, n = 16, 480000
g = torch.Generator(device=dev).manual_seed(0)
wave = 0.1 * torch.randn(B, n, device=dev, generator=g)
lengths = torch.tensor([n - 16000 * (b % 4) for b in range(B)], dtype=torch.int32, device=dev)
bank = NoiseBank([0.3 * torch.randn(16000 * s, generator=torch.Generator().manual_seed(s)) for s in (7, 20, 45, 60)], dev)
mixer = AudioAugment(noise=bank, snr_db=(0.0, 20.0))
out, scratch = torch.empty_like(wave), wave.clone()
lm80, lm128 = WhisperLogMel(dev, n_mels=80), WhisperLogMel(dev, n_mels=128)
mel80, mel128 = lm80(wave), lm128(wave)
copy80, copy128 = torch.empty_like(mel80), torch.empty_like(mel128)
masker = AudioAugment(time_masks=2, time_width=100, time_ratio=0.2, freq_masks=2, freq_width=27)
heavy = AudioAugment(time_masks=10, time_width=100, time_ratio=1.0, freq_masks=2, freq_width=27)
valid = torch.clamp((lengths + 159) // 160, max=3000).to(torch.int32)

legs = [
    ("copy                 16 x 480000 f32", lambda: out.copy_(wave)),
    ("wave_add_noise       out of place", lambda: mixer.wave(wave, lengths, 5, out=out)),
    ("wave_add_noise       in place", lambda: mixer.wave(scratch, lengths, 5, out=scratch)),
    ("logmel               n_mels 80", lambda: lm80(wave, out=mel80)),
    ("logmel               n_mels 128", lambda: lm128(wave, out=mel128)),
    ("copy                 [16, 80, 3000] f32", lambda: copy80.copy_(mel80)),
    ("spec_augment         [16, 80, 3000]  2 + 2 masks", lambda: masker.features(mel80, valid, 5)),
    ("spec_augment         [16, 80, 3000] 10 + 2 masks", lambda: heavy.features(mel80, valid, 5)),
    ("copy                 [16, 128, 3000] f32", lambda: copy128.copy_(mel128)),
    ("spec_augment         [16, 128, 3000]  2 + 2 masks", lambda: masker.features(mel128, valid, 5)),
]
# wave_add_noise and spec_augment allocate their info / spans tensor per call (torch's caching allocator: no device call after the first
# round), as the trainer's call does; the in-place mix leg keeps adding noise to its scratch copy, which changes no access pattern
rounds = [[timed(fn) for _, fn in legs] for _ in range(5)]
print(f"B = {B}, n = {n} samples (clip lengths 27 .. 30 s), noise bank 4 recordings of 7 .. 60 s; microseconds per call, median of 5 rounds (min .. max)")
for i, (name, _) in enumerate(legs):
    ts = [r[i] for r in rounds]
    print(f"{name:<52s} {statistics.median(ts):9.1f}   ({min(ts):.1f} .. {max(ts):.1f})")
