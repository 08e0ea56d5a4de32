"""Restatement of the visual augmentation (csrc/video_augment.hip; the rule is in include/avllm.h under "visual augmentation") in Python
integers and numpy, written from the header text: the draw of a clip on the hash restatement of tests/refs64_augment.py, and the whole pipeline
as oracle.preprocess.pil_bicubic_resize_u8 -> crop -> flip -> clip_normalize_lut -> masks.  Also the case list the GPU tests run
(tests/test_video_augment_gpu.py) and the planted defects that tests/test_video_augment_refs_cpu.py shows it to be sensitive to; nothing here
depends on the kernels."""
import math

import numpy as np

from oracle import preprocess as OP
from refs64_augment import M32, SPEC_SALT, as_f32, av_pair_hash, threshold

VIDEO_SALT = 0x76696465
MAX_MASKS = 16


def resized_shape(H, W, resize):
    """The shortest-edge rule: short edge -> resize, long edge -> int(resize * long / short).  -> (newH, newW)."""
    return OP.clip_resize_shape(H, W, resize)


def video_draw(clip, seed, N, newH, newW, image, random_crop=True, p_flip=0.5, n_time=0, time_width=0, time_ratio=1.0, salt=VIDEO_SALT):
    """The draw of the clip with batch index `clip` and N frames for the launch seed `seed` (seed_dev word + by-value seed, mod 2^32):
    dict(left, top, flip, spans [(start, w)] * n_time, masked = the frames in the union of the spans)."""
    s = (seed + salt) & M32
    h = lambda j: av_pair_hash(s, 64 * clip + j)      # noqa: E731
    left = (h(0) * (newW - image + 1)) >> 32 if random_crop else (newW - image) // 2
    top = (h(1) * (newH - image + 1)) >> 32 if random_crop else (newH - image) // 2
    flip = int((h(2) >> 8) < threshold(p_flip))
    wmax = min(int(time_width), int(math.floor(as_f32(time_ratio) * N)))
    spans = []
    for m in range(n_time):
        w = (h(4 + 2 * m) * (wmax + 1)) >> 32
        spans.append(((h(5 + 2 * m) * (N - w + 1)) >> 32, w))
    return {"left": left, "top": top, "flip": flip, "spans": spans, "masked": int(masked_frames(spans, N).sum())}


def masked_frames(spans, N):
    m = np.zeros(N, dtype=bool)
    for start, w in spans:
        m[start:start + w] = True
    return m


def resize_clip(frames, resize):
    """R_n for every frame: uint8 [N, newH, newW, 3]."""
    frames = np.asarray(frames, dtype=np.uint8)
    nh, nw = resized_shape(frames.shape[1], frames.shape[2], resize)
    return np.stack([OP.pil_bicubic_resize_u8(f, nh, nw) for f in frames])


def apply(resized, draw, image, fill=0.0):
    """The pipeline behind the resize: crop, then flip, then the table, then the masks.  resized uint8 [N, newH, newW, 3] -> float32
    [N, 3, image, image]."""
    t, l = draw["top"], draw["left"]
    u8 = resized[:, t:t + image, l:l + image]
    if draw["flip"]:
        u8 = u8[:, :, ::-1]
    lut = OP.clip_normalize_lut()
    out = np.stack([lut[c][u8[..., c]] for c in range(3)], axis=1).astype(np.float32)
    out[masked_frames(draw["spans"], resized.shape[0])] = np.float32(fill)
    return out


def augment_clip(frames, clip, seed, resize, image, random_crop=True, p_flip=0.5, n_time=0, time_width=0, time_ratio=1.0, fill=0.0, resized=None):
    """One clip through the header's rule -> (out float32 [N, 3, image, image], the draw).  resized: resize_clip(frames, resize) when the
    caller has it already (it depends on nothing drawn)."""
    if resized is None:
        resized = resize_clip(frames, resize)
    N, nh, nw = resized.shape[:3]
    d = video_draw(clip, seed, N, nh, nw, image, random_crop, p_flip, n_time, time_width, time_ratio)
    return apply(resized, d, image, fill), d


def to_bf16_bits(x):
    """float32 -> the bits of the nearest bfloat16, ties to even (the device's float -> bf16 conversion of a finite value), as uint16."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def pixels_augment(video, nframes, seed, first_clip=0, p_flip=0.5, n_time=0, time_width=0, time_ratio=1.0, fill=0.0):
    """The in-place entry on a copy: video [B, F, 3, S, S] (any dtype; cells are moved or overwritten, nothing is computed) ->
    (out, [draw per clip]).  `fill` is written as given: the caller converts it to the tensor's dtype."""
    out = np.array(video, copy=True)
    B, F = out.shape[:2]
    draws = []
    for b in range(B):
        N = F if nframes is None else max(0, min(F, int(nframes[b])))
        d = video_draw(first_clip + b, seed, N, 1, 1, 1, False, p_flip, n_time, time_width, time_ratio)
        d["left"] = d["top"] = -1
        m = masked_frames(d["spans"], N)
        if d["flip"]:
            out[b, :N][~m] = out[b, :N][~m][..., ::-1]
        out[b, :N][m] = fill
        draws.append(d)
    return out, draws


# ---------------------------------------------------------------- the cases of the GPU file
FILL = -1.75                                     # exact in bfloat16 and not a value of the table
AUG = dict(random_crop=True, p_flip=0.5, n_time=3, time_width=3, time_ratio=0.6)
# name -> (N, H, W, resize, image): vector forms landscape / portrait / upscale, the scalar forms (image % 4 != 0), a row too wide for the
# staged horizontal pass (64 rows of 3 * 324 bytes > 60 KiB of LDS at image 16), one frame, and no room to crop
SHAPES = {
    "landscape": (5, 37, 53, 20, 16),
    "portrait": (5, 53, 37, 20, 16),
    "upscale": (5, 12, 12, 20, 16),
    "scalar": (5, 41, 41, 18, 15),
    "wide": (2, 4, 324, 20, 16),
    "one": (1, 37, 53, 20, 16),
    "tight": (5, 64, 48, 24, 24),
    "tight16": (3, 37, 53, 16, 16),
}
# (shape, seed, clip), found by search in this file alone (find_cases): between them they hold both flip values, left and top at 0 and at
# their maximum, a zero-width span, a span ending at N, two overlapping spans, and N = 1
CASES = [
    ("landscape", 0, 0), ("landscape", 0, 1), ("landscape", 1, 3), ("landscape", 2, 3),
    ("portrait", 0, 0), ("portrait", 0, 1), ("portrait", 0, 6), ("portrait", 2, 4),
    ("upscale", 0, 0), ("upscale", 2, 3),
    ("scalar", 0, 0), ("scalar", 0, 1), ("scalar", 2, 3),
    ("wide", 0, 0), ("wide", 0, 1),
    ("one", 0, 0), ("one", 0, 1),
    ("tight", 0, 0), ("tight", 0, 4), ("tight16", 1, 1),
]


def case_frames(shape):
    """The clip of a shape: seeded uint8 noise over a gradient (every frame and every column distinct, so no crop, flip or span goes unseen)."""
    N, H, W, _, _ = SHAPES[shape]
    g = np.random.default_rng(sorted(SHAPES).index(shape))
    ramp = (np.arange(W)[None, :, None] * 3 + np.arange(H)[:, None, None] * 2 + np.arange(3)[None, None, :] * 40)
    noise = g.integers(0, 96, (N, H, W, 3))
    return ((ramp[None] + noise + 17 * np.arange(N)[:, None, None, None]) % 256).astype(np.uint8)


def case_draw(shape, seed, clip, **over):
    N, H, W, resize, image = SHAPES[shape]
    nh, nw = resized_shape(H, W, resize)
    kw = dict(AUG, **over)
    return video_draw(clip, seed, N, nh, nw, image, kw["random_crop"], kw["p_flip"], kw["n_time"], kw["time_width"], kw["time_ratio"])


def coverage(cases=None):
    """What the case list holds, as a dict of booleans."""
    got = dict.fromkeys(("flip0", "flip1", "left0", "leftmax", "top0", "topmax", "zero_width", "ends_at_N", "overlap", "N1"), False)
    for shape, seed, clip in (CASES if cases is None else cases):
        N, H, W, resize, image = SHAPES[shape]
        nh, nw = resized_shape(H, W, resize)
        d = case_draw(shape, seed, clip)
        got["flip1" if d["flip"] else "flip0"] = True
        if nw > image:
            got["left0"] |= d["left"] == 0
            got["leftmax"] |= d["left"] == nw - image
        if nh > image:
            got["top0"] |= d["top"] == 0
            got["topmax"] |= d["top"] == nh - image
        sp = d["spans"]
        got["zero_width"] |= any(w == 0 for _, w in sp)
        got["ends_at_N"] |= any(w > 0 and s + w == N for s, w in sp)
        got["overlap"] |= any(a[1] > 0 and b[1] > 0 and a[0] < b[0] + b[1] and b[0] < a[0] + a[1] for i, a in enumerate(sp) for b in sp[i + 1:])
        got["N1"] |= N == 1
    return got


def find_cases(shape, want, seeds=range(64), clips=range(8)):
    """The first (seed, clip) of `shape` whose draw satisfies want(draw, N, newH, newW, image): how CASES was chosen."""
    N, H, W, resize, image = SHAPES[shape]
    nh, nw = resized_shape(H, W, resize)
    for seed in seeds:
        for clip in clips:
            if want(case_draw(shape, seed, clip), N, nh, nw, image):
                return seed, clip
    return None


# ---------------------------------------------------------------- planted defects: the pipeline with one thing wrong
def defective(kind, frames, clip, seed, resize, image, fill=FILL, F_pad=None, resized=None, **kw):
    """The output of a pipeline with the planted defect `kind`, for comparison with augment_clip's."""
    kw = dict(AUG, **kw)
    if resized is None:
        resized = resize_clip(frames, resize)
    N, nh, nw = resized.shape[:3]
    draw = lambda **o: video_draw(clip, seed, o.pop("N", N), o.pop("nh", nh), o.pop("nw", nw), image, kw["random_crop"], kw["p_flip"],      # noqa: E731
                                  kw["n_time"], kw["time_width"], kw["time_ratio"], **o)
    d = draw()
    if kind == "flip_before_crop":
        r = resized[:, :, ::-1] if d["flip"] else resized
        return apply(r, dict(d, flip=0), image, fill)
    if kind == "crop_range_without_plus_one":
        s = (seed + VIDEO_SALT) & M32
        d = dict(d, left=(av_pair_hash(s, 64 * clip) * (nw - image)) >> 32, top=(av_pair_hash(s, 64 * clip + 1) * (nh - image)) >> 32)
        return apply(resized, d, image, fill)
    if kind == "left_top_exchanged":
        s = (seed + VIDEO_SALT) & M32
        d = dict(d, left=(av_pair_hash(s, 64 * clip + 1) * (nw - image + 1)) >> 32, top=(av_pair_hash(s, 64 * clip) * (nh - image + 1)) >> 32)
        return apply(resized, d, image, fill)
    if kind == "flip_per_frame":
        s = (seed + VIDEO_SALT) & M32
        out = apply(resized, dict(d, flip=0), image, fill)
        m = masked_frames(d["spans"], N)
        for n in range(N):
            if not m[n] and (av_pair_hash(s, 64 * clip + 2 + 64 * 1024 * n) >> 8) < threshold(kw["p_flip"]):
                out[n] = out[n][..., ::-1]
        return out
    if kind == "span_extent_from_padded_F":
        F = F_pad if F_pad is not None else N + 3
        dF = draw(N=F)
        return apply(resized, dict(d, spans=[(s0, w) for s0, w in dF["spans"]]), image, fill)
    if kind == "span_one_frame_late":
        return apply(resized, dict(d, spans=[(s0 + 1, w) for s0, w in d["spans"]]), image, fill)
    if kind == "fill_before_lut":
        out = apply(resized, dict(d, spans=[]), image, fill)
        lut = OP.clip_normalize_lut()
        v = int(np.clip(round(fill), 0, 255))
        for n in np.nonzero(masked_frames(d["spans"], N))[0]:
            for c in range(3):
                out[n, c] = lut[c][v]
        return out
    if kind == "audio_salt":
        return apply(resized, draw(salt=SPEC_SALT), image, fill)
    raise KeyError(kind)


DEFECTS = ("flip_before_crop", "crop_range_without_plus_one", "left_top_exchanged", "flip_per_frame", "span_extent_from_padded_F",
           "span_one_frame_late", "fill_before_lut", "audio_salt")
