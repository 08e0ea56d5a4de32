"""tests/refs_video_augment.py against things that do not depend on it: Pillow's own resize at every shape the GPU file uses, the oracle's
CLIP pipeline in the identity configuration, the coverage of the GPU file's case list, planted defects (each must change the output of some
case of that list), and the frequencies of the draw."""
import math

import numpy as np
import pytest

import refs_video_augment as RV
from oracle import preprocess as OP
from refs64_augment import av_pair_hash, threshold


@pytest.fixture(scope="module")
def resized():
    return {sh: RV.resize_clip(RV.case_frames(sh), RV.SHAPES[sh][3]) for sh in RV.SHAPES}


@pytest.mark.parametrize("hwr", [(24, 32, 20), (24, 32, 56)], ids=["toy-20", "toy-56"])
def test_resize_restatement_is_pillows_at_the_pipeline_shapes(hwr):
    """The (H, W, resize) that tests/test_video_augment_pipeline_gpu.py feeds to the restatement: the toy set's 24 x 32 frames."""
    pytest.importorskip("PIL")
    from PIL import Image
    H, W, resize = hwr
    frames = np.random.RandomState(5).randint(0, 256, (3, H, W, 3), dtype=np.uint8)
    nh, nw = RV.resized_shape(H, W, resize)
    got = RV.resize_clip(frames, resize)
    for n in range(3):
        assert np.array_equal(got[n], np.asarray(Image.fromarray(frames[n]).resize((nw, nh), Image.BICUBIC))), (hwr, n)


@pytest.mark.parametrize("shape", sorted(RV.SHAPES))
def test_resize_restatement_is_pillows(shape, resized):
    pytest.importorskip("PIL")
    from PIL import Image
    N, H, W, resize, _ = RV.SHAPES[shape]
    nh, nw = RV.resized_shape(H, W, resize)
    short, long_ = min(H, W), max(H, W)
    assert min(nh, nw) == resize and max(nh, nw) == int(resize * long_ / short)
    frames = RV.case_frames(shape)
    for n in range(N):
        want = np.asarray(Image.fromarray(frames[n]).resize((nw, nh), Image.BICUBIC))
        assert np.array_equal(resized[shape][n], want), (shape, n)


@pytest.mark.parametrize("shape", ["landscape", "portrait", "upscale", "scalar", "tight"])
def test_identity_configuration_is_the_oracles_pipeline(shape):
    N, H, W, _, image = RV.SHAPES[shape]
    frames = RV.case_frames(shape)
    out, d = RV.augment_clip(frames, 3, 99, image, image, random_crop=False, p_flip=0.0, n_time=0)
    nh, nw = RV.resized_shape(H, W, image)
    assert (d["left"], d["top"], d["flip"], d["spans"], d["masked"]) == ((nw - image) // 2, (nh - image) // 2, 0, [], 0)
    for n in range(N):
        assert np.array_equal(out[n].view(np.uint32), OP.clip_pixel_values(frames[n], image).view(np.uint32)), (shape, n)


def test_case_list_holds_every_edge():
    got = RV.coverage()
    assert all(got.values()), got
    assert {sh for sh, _, _ in RV.CASES} == set(RV.SHAPES)
    for shape, seed, clip in RV.CASES:                    # every draw stays inside its ranges
        N, H, W, resize, image = RV.SHAPES[shape]
        nh, nw = RV.resized_shape(H, W, resize)
        d = RV.case_draw(shape, seed, clip)
        assert 0 <= d["left"] <= nw - image and 0 <= d["top"] <= nh - image
        assert all(0 <= w <= min(3, math.floor(0.6 * N)) and 0 <= s and s + w <= N for s, w in d["spans"])


@pytest.mark.parametrize("kind", RV.DEFECTS)
def test_planted_defect_shows_on_the_case_list(kind, resized):
    hits = 0
    for shape, seed, clip in RV.CASES:
        _, _, _, resize, image = RV.SHAPES[shape]
        good, _ = RV.augment_clip(None, clip, seed, resize, image, fill=RV.FILL, resized=resized[shape], **RV.AUG)
        bad = RV.defective(kind, None, clip, seed, resize, image, resized=resized[shape])
        hits += not np.array_equal(good.view(np.uint32), bad.view(np.uint32))
    assert hits > 0, kind


def test_draw_frequencies_over_4096_clips():
    n, seed, p = 4096, 12345, 0.3
    newH, newW, image = 20, 28, 16
    draws = [RV.video_draw(c, seed, 10, newH, newW, image, True, p, 0) for c in range(n)]
    flips = sum(d["flip"] for d in draws)
    pq = threshold(p) / 2.0 ** 24
    assert abs(flips - n * pq) <= 4.0 * math.sqrt(n * pq * (1 - pq)), flips
    assert {d["left"] for d in draws} == set(range(newW - image + 1)) and {d["top"] for d in draws} == set(range(newH - image + 1))
    # left, top and flip come from three different words of the stream
    s = (seed + RV.VIDEO_SALT) & 0xFFFFFFFF
    assert draws[7]["left"] == (av_pair_hash(s, 64 * 7) * 13) >> 32 and draws[7]["top"] == (av_pair_hash(s, 64 * 7 + 1) * 5) >> 32
    assert draws[7]["flip"] == int((av_pair_hash(s, 64 * 7 + 2) >> 8) < threshold(p))


def test_in_place_restatement_matches_the_fused_one():
    """Resize == image and no crop: the fused pipeline of a clip equals the plain pipeline followed by the in-place rule at the same keys."""
    shape = "tight16"
    N, H, W, resize, image = RV.SHAPES[shape]
    frames = RV.case_frames(shape)
    kw = dict(p_flip=0.5, n_time=2, time_width=2, time_ratio=1.0)
    F = N + 2
    for clip in range(6):
        fused, d = RV.augment_clip(frames, clip, 21, resize, image, random_crop=False, fill=RV.FILL, **kw)
        plain = np.full((1, F, 3, image, image), np.float32(7.5))
        plain[0, :N] = np.stack([OP.clip_pixel_values(f, image) for f in frames])
        out, draws = RV.pixels_augment(plain, [N], 21, first_clip=clip, fill=np.float32(RV.FILL), **kw)
        assert np.array_equal(out[0, :N], fused) and (out[0, N:] == 7.5).all()
        assert (draws[0]["flip"], draws[0]["spans"], draws[0]["masked"]) == (d["flip"], d["spans"], d["masked"])
