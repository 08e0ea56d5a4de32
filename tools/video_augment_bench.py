#!/usr/bin/env python3
"""Times the visual augmentation kernels (csrc/video_augment.hip) against the plain call they extend, in one process per workload:
16 clips x 125 frames of 96x96 and of 224x224 uint8, resize 256 -> image 224 and resize 224 -> image 224, float32 output.  Legs, alternated
within a round: avllm_clip_preproc of the same frames (the yardstick), the fused call with everything on (random crop, flip_prob 0.5, 2 time
masks of up to 25 frames), the same without masks with the flip forced off and forced on (does the flip cost anything?), and -- once, beside
the 224x224 / 224 workload -- avllm_video_frames_augment in place on [16, 125, 3, 224, 224].  Five rounds, the median per leg in microseconds
PER CLIP and the round-to-round spread (min .. max); device events around 5 passes over the 16 clips.  No ratio is asserted.

Without arguments this is the driver: it starts one child per workload, each under a `timeout` of its own, and stops at the first that fails."""
import os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))

B, N, IMAGE = 16, 125, 224
WORKLOADS = [(96, 96, 256), (96, 96, 224), (224, 224, 256), (224, 224, 224)]
LIMIT_S = 120


def timed(fn, n=5):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000 / B


def child(H, W, resize):
    import torch
    from avllm.preprocess import ClipFrames, VideoAugment
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    clips = [torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(B)]
    cf = ClipFrames(dev, image=IMAGE)
    out = torch.empty(B, N, 3, IMAGE, IMAGE, dtype=torch.float32, device=dev)
    full = VideoAugment(resize=resize, random_crop=True, flip_prob=0.5, time_masks=2, time_width=25, time_ratio=0.4)
    noflip = VideoAugment(resize=resize, random_crop=True, flip_prob=0.0)
    flip = VideoAugment(resize=resize, random_crop=True, flip_prob=1.0)
    info, spans = torch.empty(B, 4, dtype=torch.int32, device=dev), torch.empty(B, 2, 2, dtype=torch.int32, device=dev)

    def fused(aug):
        def run():
            for i, c in enumerate(clips):
                aug.frames(cf, c, i, 5, out=out[i], info=info[i], spans=spans[i])
        return run

    def plain():
        for i, c in enumerate(clips):
            cf(c, out=out[i])

    legs = [(f"clip_preproc          {H}x{W} -> {IMAGE}", plain),
            (f"clip_preproc_aug      {H}x{W} -> {resize} -> {IMAGE}, crop + flip 0.5 + 2 masks", fused(full)),
            (f"clip_preproc_aug      {H}x{W} -> {resize} -> {IMAGE}, crop, never flipped", fused(noflip)),
            (f"clip_preproc_aug      {H}x{W} -> {resize} -> {IMAGE}, crop, always flipped", fused(flip))]
    if (H, W, resize) == (224, 224, 224):
        place = VideoAugment(flip_prob=0.5, time_masks=2, time_width=25, time_ratio=0.4)
        legs.append((f"video_frames_augment  in place on [{B}, {N}, 3, {IMAGE}, {IMAGE}] f32, flip 0.5 + 2 masks", lambda: place.pixels(out, None, 5)))
    rounds = [[timed(fn) for _, fn in legs] for _ in range(5)]
    for i, (name, _) in enumerate(legs):
        ts = [r[i] for r in rounds]
        print(f"{name:<86s} {statistics.median(ts):9.1f}   ({min(ts):.1f} .. {max(ts):.1f})")
    f = VideoAugment.info_fields(info)
    print(f"  last fused batch: {sum(f['flip'])} of {B} clips flipped, {sum(f['masked'])} of {B * N} frames masked")


if __name__ == "__main__":
    if len(sys.argv) == 4:
        child(*(int(v) for v in sys.argv[1:]))
        sys.exit(0)
    print(f"{B} clips x {N} frames, image {IMAGE}, float32 output; microseconds per clip, median of 5 rounds (min .. max)")
    sys.stdout.flush()
    for H, W, resize in WORKLOADS:
        rc = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), str(H), str(W), str(resize)]).returncode
        if rc != 0:
            print(f"workload {H}x{W} resize {resize}: exit status {rc}; stopping here")
            sys.exit(rc)
