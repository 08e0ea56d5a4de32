"""The visual augmentation kernels (csrc/video_augment.hip) through the C ABI against tests/refs_video_augment.py, bit for bit.  Every output is a
view inside a sentinel-filled buffer, and info and spans are sentinel-guarded; the case list and its coverage are pinned on the CPU by
tests/test_video_augment_refs_cpu.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import refs_video_augment as RV  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm.preprocess import CLIP_MEAN, CLIP_STD  # noqa: E402

GUARD = 128                      # int16 cells in front of and behind every buffer (keeps the payload 256-byte aligned)
SENT = 0x7FC1                    # a bfloat16 NaN; two of them are a float32 NaN with a payload
PAD_BITS = {torch.float32: 0x7FC01234, torch.bfloat16: 0x7FD2}      # NaNs with payloads, planted in padding frames
MEAN, STD = (ctypes.c_float * 3)(*CLIP_MEAN), (ctypes.c_float * 3)(*CLIP_STD)
DTYPES = [torch.float32, torch.bfloat16]
ERR_ARG = 1


class Guarded:
    """`count` cells of `dtype` (float32, bfloat16 or int32) between two guards, everything holding SENT until somebody writes."""

    def __init__(self, dev, count, dtype):
        self.count, self.dtype, self.cell = count, dtype, 1 if dtype == torch.bfloat16 else 2
        self.n16 = count * self.cell
        self.buf = torch.full((2 * GUARD + self.n16,), SENT, dtype=torch.int16, device=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 2 * GUARD

    def tensor(self):
        return self.buf[GUARD:GUARD + self.n16].view(self.dtype)

    def put_bits(self, bits):
        a = np.ascontiguousarray(bits)
        self.buf[GUARD:GUARD + self.n16].copy_(torch.from_numpy(a.view(np.int16).reshape(-1)).to(self.buf.device))
        return self

    def bits(self):
        """The payload's bits (uint32 for 4-byte cells, uint16 for bfloat16); asserts that both guards still hold the sentinel."""
        host = self.buf.cpu().numpy().view(np.uint16)
        assert (host[:GUARD] == SENT).all() and (host[GUARD + self.n16:] == SENT).all(), "a guard was written"
        body = np.ascontiguousarray(host[GUARD:GUARD + self.n16])
        return body if self.cell == 1 else body.view(np.uint32)

    def untouched(self):
        return bool((self.bits().view(np.uint16) == SENT).all())


_plans = {}


def aug_plan(dev, H, W, resize, image):
    key = (H, W, resize, image)
    if key not in _plans:
        lib = L.load()
        nbytes = lib.avllm_clip_preproc_aug_plan_bytes(H, W, resize, image)
        assert nbytes > 0
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        L.check(lib.avllm_clip_preproc_aug_plan_init(L.ptr(buf), H, W, resize, image, MEAN, STD))
        _plans[key] = buf
    return _plans[key]


def plain_plan(dev, H, W, image):
    key = (H, W, image)
    if key not in _plans:
        lib = L.load()
        buf = torch.empty(lib.avllm_clip_preproc_plan_bytes(H, W, image), dtype=torch.uint8, device=dev)
        L.check(lib.avllm_clip_preproc_plan_init(L.ptr(buf), H, W, image, MEAN, STD))
        _plans[key] = buf
    return _plans[key]


def fused(dev, frames, resize, image, clip, seed, dtype=torch.float32, random_crop=True, p_flip=0.5, n_time=0, time_width=0, time_ratio=1.0,
          fill=RV.FILL, seed_dev=None, expect=0, ws_short=0, plan=None):
    """One avllm_clip_preproc_aug call.  -> (out bits [N, 3, image, image], info [4], spans [n_time, 2]); with expect != 0 the call must return
    that code and leave the output sentinel alone (-> the error text)."""
    lib = L.load()
    N, H, W, _ = frames.shape
    src = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    out = Guarded(dev, N * 3 * image * image, dtype)
    info, spans = Guarded(dev, 4, torch.int32), Guarded(dev, max(1, 2 * max(0, min(n_time, 16))), torch.int32)
    need = max(256, lib.avllm_clip_preproc_aug_workspace_bytes(N, H, W, resize, image))
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    plan = aug_plan(dev, H, W, resize, image) if plan is None else plan
    rc = lib.avllm_clip_preproc_aug(L.ptr(plan), L.ptr(src), N, H, W, resize, image, clip, int(random_crop), p_flip, n_time, time_width, time_ratio,
                                    fill, seed & 0xFFFFFFFF, L.ptr(seed_dev), out.ptr, L.dt_of(out.tensor()), info.ptr, spans.ptr, L.ptr(ws),
                                    need - ws_short, L.stream_ptr())
    torch.cuda.synchronize()
    if expect:
        assert rc == expect, (rc, lib.avllm_last_error())
        assert out.untouched() and info.untouched() and spans.untouched(), "a refused call wrote"
        return lib.avllm_last_error().decode()
    L.check(rc)
    sp = spans.bits().view(np.int32)
    assert n_time > 0 or sp.view(np.uint16)[0] == SENT
    return out.bits().reshape(N, 3, image, image), info.bits().view(np.int32).tolist(), sp[:2 * n_time].reshape(n_time, 2).tolist()


def plain(dev, frames, image, dtype):
    """avllm_clip_preproc of the same frames -> bits [N, 3, image, image]."""
    lib = L.load()
    N, H, W, _ = frames.shape
    src = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    out = Guarded(dev, N * 3 * image * image, dtype)
    need = lib.avllm_clip_preproc_workspace_bytes(N, H, W, image)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    L.check(lib.avllm_clip_preproc(L.ptr(plain_plan(dev, H, W, image)), L.ptr(src), N, H, W, image, out.ptr,
                                   L.F32 if dtype == torch.float32 else L.BF16, L.ptr(ws), need, L.stream_ptr()))
    torch.cuda.synchronize()
    return out.bits().reshape(N, 3, image, image)


def want_bits(ref32, dtype):
    return ref32.view(np.uint32) if dtype == torch.float32 else RV.to_bf16_bits(ref32)


@pytest.fixture(scope="module")
def resized():
    """The reference's resize of every shape's clip: computed once, shared, never written."""
    out = {sh: RV.resize_clip(RV.case_frames(sh), RV.SHAPES[sh][3]) for sh in RV.SHAPES}
    for r in out.values():
        r.setflags(write=False)
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", RV.CASES, ids=lambda c: f"{c[0]}-s{c[1]}-c{c[2]}")
def test_fused_call_equals_the_restatement(dev, case, dtype, resized):
    shape, seed, clip = case
    N, H, W, resize, image = RV.SHAPES[shape]
    ref, d = RV.augment_clip(None, clip, seed, resize, image, fill=RV.FILL, resized=resized[shape], **RV.AUG)
    got, info, spans = fused(dev, RV.case_frames(shape), resize, image, clip, seed, dtype, **RV.AUG)
    assert info == [d["left"], d["top"], d["flip"], d["masked"]] and spans == [list(s) for s in d["spans"]]
    bad = np.argwhere(got != want_bits(ref, dtype))
    assert bad.size == 0, f"{len(bad)} of {got.size} cells differ: frames {sorted(set(bad[:, 0]))}, rows {sorted(set(bad[:, 2]))}, columns {sorted(set(bad[:, 3]))}"


def test_a_single_masked_frame(dev, resized):
    """N = 1 with a ratio that admits a span of the one frame: the whole output is the fill."""
    N, H, W, resize, image = RV.SHAPES["one"]
    kw = dict(random_crop=True, p_flip=0.5, n_time=1, time_width=1, time_ratio=1.0)
    seen = set()
    for clip in range(6):
        ref, d = RV.augment_clip(None, clip, 3, resize, image, fill=RV.FILL, resized=resized["one"], **kw)
        got, info, spans = fused(dev, RV.case_frames("one"), resize, image, clip, 3, **kw)
        assert info[3] == d["masked"] and spans == [list(s) for s in d["spans"]] and np.array_equal(got, ref.view(np.uint32))
        seen.add(d["masked"])
    assert seen == {0, 1}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", sorted(RV.SHAPES))
def test_identity_configuration_is_the_plain_call(dev, shape, dtype):
    N, H, W, _, image = RV.SHAPES[shape]
    frames = RV.case_frames(shape)
    got, info, _ = fused(dev, frames, image, image, 5, 77, dtype, random_crop=False, p_flip=0.0, n_time=0)
    nh, nw = RV.resized_shape(H, W, image)
    assert info == [(nw - image) // 2, (nh - image) // 2, 0, 0]
    assert np.array_equal(got, plain(dev, frames, image, dtype))


def frames_augment(dev, video_bits, dtype, nframes, seed, first_clip=0, p_flip=0.5, n_time=0, time_width=0, time_ratio=1.0, fill=RV.FILL,
                   seed_dev=None):
    """One avllm_video_frames_augment call on a guarded copy of video_bits [B, F, 3, S, S] -> (bits, info [B, 4], spans [B, n_time, 2])."""
    B, F, _, S, _ = video_bits.shape
    buf = Guarded(dev, video_bits.size, dtype).put_bits(video_bits)
    info, spans = Guarded(dev, 4 * B, torch.int32), Guarded(dev, max(1, 2 * B * n_time), torch.int32)
    nf = None if nframes is None else torch.tensor(nframes, dtype=torch.int32, device=dev)
    L.check(L.load().avllm_video_frames_augment(buf.ptr, L.F32 if dtype == torch.float32 else L.BF16, B, F, S, L.ptr(nf), first_clip, p_flip, n_time,
                                                time_width, time_ratio, fill, seed & 0xFFFFFFFF, L.ptr(seed_dev), info.ptr, spans.ptr, L.stream_ptr()))
    torch.cuda.synchronize()
    return (buf.bits().reshape(video_bits.shape), info.bits().view(np.int32).reshape(B, 4).tolist(),
            spans.bits().view(np.int32)[:2 * B * n_time].reshape(B, n_time, 2).tolist())


def fill_bits(dtype):
    return want_bits(np.array([RV.FILL], np.float32), dtype)[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", ["tight16", "scalar"])
def test_the_two_entries_agree(dev, shape, dtype):
    """The fused call without a crop = the plain call into a padded batch, then the in-place entry: pixels, flip, masked and spans."""
    _, H, W, _, image = RV.SHAPES[shape]
    all_frames = RV.case_frames(shape)
    counts, F, first = [all_frames.shape[0], 1, 2, all_frames.shape[0] - 1], all_frames.shape[0] + 1, 2
    kw = dict(p_flip=0.5, n_time=2, time_width=2, time_ratio=1.0)
    np_dt = np.uint32 if dtype == torch.float32 else np.uint16
    batch = np.full((len(counts), F, 3, image, image), PAD_BITS[dtype], dtype=np_dt)
    for b, n in enumerate(counts):
        batch[b, :n] = plain(dev, all_frames[:n], image, dtype)
    got, info, spans = frames_augment(dev, batch, dtype, counts, 31, first_clip=first, **kw)
    flips = set()
    for b, n in enumerate(counts):
        one, i1, s1 = fused(dev, all_frames[:n], image, image, first + b, 31, dtype, random_crop=False, **kw)
        assert np.array_equal(got[b, :n], one), (b, n)
        assert (got[b, n:] == PAD_BITS[dtype]).all(), "a padding frame was written"
        assert info[b] == [-1, -1, i1[2], i1[3]] and spans[b] == s1
        flips.add(i1[2])
    assert flips == {0, 1}


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("S", [16, 15, 12])
def test_in_place_entry_moves_bits_and_leaves_the_rest(dev, S, dtype):
    """Planted NaN payloads and -0 in every cell: what flips is moved bit for bit, what is masked holds the fill, padding frames and the clips
    that neither flip nor are masked keep every bit.  S = 16 / 12: vector forms with an even / odd count of groups, 15: the scalar form."""
    B, F, counts = 6, 5, [5, 0, 3, 5, 1, 4]
    g = np.random.default_rng(S)
    np_dt = np.uint32 if dtype == torch.float32 else np.uint16
    video = g.integers(0, 2 ** (32 if dtype == torch.float32 else 16), (B, F, 3, S, S), dtype=np.uint64).astype(np_dt)
    video[:, :, 0, 0, :4] = [PAD_BITS[dtype], 0x80000000 >> (0 if dtype == torch.float32 else 16), 0, PAD_BITS[dtype] + 1]
    kw = dict(p_flip=0.5, n_time=2, time_width=2, time_ratio=0.5)
    want, draws = RV.pixels_augment(video, counts, 2, first_clip=1, fill=fill_bits(dtype), **kw)      # seed 2: found in the restatement
    got, info, spans = frames_augment(dev, video, dtype, counts, 2, first_clip=1, **kw)
    assert np.array_equal(got, want)
    assert info == [[-1, -1, d["flip"], d["masked"]] for d in draws] and spans == [[list(s) for s in d["spans"]] for d in draws]
    assert {d["flip"] for d in draws} == {0, 1} and any(d["masked"] == 0 and not d["flip"] for d in draws) and any(d["masked"] for d in draws)
    # nframes NULL counts every frame; masks alone (no flip) and a flip alone
    for over in (dict(p_flip=0.0), dict(n_time=0), dict(p_flip=1.0, n_time=0)):
        k2 = dict(kw, **over)
        want, draws = RV.pixels_augment(video, None, 8, fill=fill_bits(dtype), **k2)
        got, info, _ = frames_augment(dev, video, dtype, None, 8, **k2)
        assert np.array_equal(got, want) and [r[2:] for r in info] == [[d["flip"], d["masked"]] for d in draws]


def test_in_place_entry_without_work_launches_nothing(dev):
    lib = L.load()
    assert lib.avllm_video_frames_augment(None, L.F32, 4, 5, 16, None, 0, 0.0, 0, 0, 1.0, 0.0, 1, None, None, None, L.stream_ptr()) == 0
    assert lib.avllm_video_frames_augment(None, L.F32, 4, 5, 16, None, 0, 1e-9, 0, 7, 1.0, 0.0, 1, None, None, None, L.stream_ptr()) == 0      # rounds to 0
    assert lib.avllm_video_frames_augment(None, L.F32, 4, 5, 16, None, 0, 0.5, 0, 0, 1.0, 0.0, 1, None, None, None, L.stream_ptr()) == ERR_ARG
    assert b"pixels NULL" in lib.avllm_last_error()
    for bad, word in ((dict(p_flip=1.5), "p_flip"), (dict(n_time=17), "n_time"), (dict(time_width=-1), "max_time_width"),
                      (dict(time_ratio=-0.5), "max_time_ratio"), (dict(first_clip=-1), "first_clip")):
        kw = dict(dict(p_flip=0.5, n_time=1, time_width=1, time_ratio=1.0, first_clip=0), **bad)
        buf = Guarded(dev, 2 * 3 * 3 * 16 * 16, torch.float32)
        rc = lib.avllm_video_frames_augment(buf.ptr, L.F32, 2, 3, 16, None, kw["first_clip"], kw["p_flip"], kw["n_time"], kw["time_width"],
                                            kw["time_ratio"], 0.0, 1, None, buf.ptr, buf.ptr, L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == ERR_ARG and word in lib.avllm_last_error().decode() and buf.untouched(), word


def test_repeat_seed_word_and_clip(dev):
    shape = "landscape"
    N, H, W, resize, image = RV.SHAPES[shape]
    frames = RV.case_frames(shape)
    a = fused(dev, frames, resize, image, 2, 0x10, **RV.AUG)
    b = fused(dev, frames, resize, image, 2, 0x10, **RV.AUG)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:]                                    # a repeated launch repeats its bits
    word = torch.tensor([0xFFFFFFF0 - 2 ** 32], dtype=torch.int32, device=dev)             # the bits of 0xFFFFFFF0
    c = fused(dev, frames, resize, image, 2, 0x20, seed_dev=word, **RV.AUG)                 # 0xFFFFFFF0 + 0x20 wraps to 0x10
    assert np.array_equal(a[0], c[0]) and a[1:] == c[1:]
    draws = {tuple(fused(dev, frames, resize, image, clip, 0x10, **RV.AUG)[1]) for clip in range(6)}
    assert len(draws) > 1                                                                    # one seed, other clips: other draws
    vid = np.zeros((1, 5, 3, 16, 16), np.uint32)
    assert frames_augment(dev, vid, torch.float32, None, 0x20, first_clip=2, seed_dev=word, n_time=3, time_width=3, time_ratio=0.6)[1:] == \
        frames_augment(dev, vid, torch.float32, None, 0x10, first_clip=2, n_time=3, time_width=3, time_ratio=0.6)[1:]


def test_refusals_name_the_argument_and_write_nothing(dev):
    lib = L.load()
    N, H, W, resize, image = RV.SHAPES["landscape"]
    frames = RV.case_frames("landscape")
    good = aug_plan(dev, H, W, resize, image)
    ok = dict(random_crop=True, p_flip=0.5, n_time=2, time_width=2, time_ratio=0.5)
    assert lib.avllm_clip_preproc_aug_plan_bytes(H, W, image - 1, image) == 0
    scratch = torch.empty(4096, dtype=torch.uint8, device=dev)
    assert lib.avllm_clip_preproc_aug_plan_init(L.ptr(scratch), H, W, image - 1, image, MEAN, STD) == ERR_ARG and b"resize" in lib.avllm_last_error()
    for kw, word in ((dict(ok, p_flip=1.25), "p_flip"), (dict(ok, p_flip=-0.1), "p_flip"), (dict(ok, p_flip=float("nan")), "p_flip"),
                     (dict(ok, n_time=17), "n_time"), (dict(ok, n_time=-1), "n_time"), (dict(ok, time_width=-1), "max_time_width"),
                     (dict(ok, time_ratio=1.5), "max_time_ratio"), (dict(ok, time_ratio=-0.25), "max_time_ratio")):
        assert word in fused(dev, frames, resize, image, 0, 1, expect=ERR_ARG, plan=good, **kw), (kw, word)
    assert "clip=-1" in fused(dev, frames, resize, image, -1, 1, expect=ERR_ARG, plan=good, **ok)
    assert "resize" in fused(dev, frames, image - 1, image, 0, 1, expect=ERR_ARG, plan=good, **ok)
    assert "workspace" in fused(dev, frames, resize, image, 0, 1, expect=ERR_ARG, plan=good, ws_short=1, **ok)
    # a plan made for another resize, another image, another frame size, and a plain plan
    assert "plan is for" in fused(dev, frames, resize + 1, image, 0, 1, expect=ERR_ARG, plan=good, **ok)
    assert "plan is for" in fused(dev, frames, resize, image - 4, 0, 1, expect=ERR_ARG, plan=good, **ok)
    assert "plan is for" in fused(dev, frames[:, :-1], resize, image, 0, 1, expect=ERR_ARG, plan=good, **ok)
    assert "not initialised" in fused(dev, frames, resize, image, 0, 1, expect=ERR_ARG, plan=plain_plan(dev, H, W, image), **ok)
