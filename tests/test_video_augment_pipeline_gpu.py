"""Visual augmentation above the kernels: VideoAugment and device_collate(video_augment=) against tests/refs_video_augment.py, the trainer's
video_augment (training batches only, a trainer without one prepares the tensors it prepared before, precomputed pixel_values take the in-place
path on a copy), and the configuration keys and train.py flags, on the tiny model with toy files written into a temporary directory."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import refs_video_augment as RV  # noqa: E402
from oracle import weights as Wt  # noqa: E402
from test_data_cpu import make_set  # noqa: E402
from test_model_gpu import make_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(resize=20, random_crop=True, flip_prob=0.5, time_masks=2, time_width=2, time_ratio=0.75, fill=-1.75)
IMAGE = 16


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    root = tmp_path_factory.mktemp("toy")
    mp, lp = make_set(root, n=4)
    return root, mp, lp


def raw_samples(toy, n=4):
    from avllm.data import AVSRDataset
    from avllm.tokenizer import ByteTokenizer
    root, mp, lp = toy
    ds = AVSRDataset(str(mp), str(lp), str(root), ByteTokenizer(512), max_video_length=4)
    return [ds[i] for i in range(n)]


def restated(samples, seed, resize=KW["resize"], image=IMAGE):
    """[(out float32 [N, 3, image, image], draw)] of the samples' clips by the header's rule with KW."""
    return [RV.augment_clip(np.asarray(s["frames"])[:4], i, seed, resize, image, KW["random_crop"], KW["flip_prob"],
                            KW["time_masks"], KW["time_width"], KW["time_ratio"], KW["fill"]) for i, s in enumerate(samples)]


def test_device_collate_is_the_restatement_clip_by_clip(dev, toy):
    from avllm.preprocess import ClipFrames, VideoAugment, WhisperLogMel, device_collate
    samples = raw_samples(toy)
    lm, cf = WhisperLogMel(dev), ClipFrames(dev, image=IMAGE)
    aug = VideoAugment(**KW)
    plain_a, plain_v = device_collate(samples, lm, cf, max_video_length=4)
    audio, video = device_collate(samples, lm, cf, max_video_length=4, video_augment=aug, seed=11)
    assert torch.equal(audio, plain_a) and video.shape == plain_v.shape and not torch.equal(video, plain_v)
    want = restated(samples, 11)
    fields = VideoAugment.info_fields(aug.last_info)
    for i, (ref, d) in enumerate(want):
        n = ref.shape[0]
        assert np.array_equal(video[i, :n].cpu().numpy().view(np.uint32), ref.view(np.uint32)), i
        assert float(video[i, n:].abs().max() if n < video.shape[1] else 0.0) == 0.0                       # padding frames stay zero
        assert (fields["left"][i], fields["top"][i], fields["flip"][i], fields["masked"][i]) == (d["left"], d["top"], d["flip"], d["masked"])
        assert aug.last_spans[i].tolist() == [list(s) for s in d["spans"]]
    assert aug.last_frames == [w[0].shape[0] for w in want]
    # one clip by hand, bf16 featurizer: the float32 result rounded
    cf16 = ClipFrames(dev, image=IMAGE, dtype=torch.bfloat16)
    one = aug.frames(cf16, samples[1]["frames"][:4], 1, 11)
    assert one.dtype == torch.bfloat16 and np.array_equal(one.view(torch.int16).cpu().numpy().view(np.uint16), RV.to_bf16_bits(want[1][0]))
    assert aug.last_info.shape == (1, 4) and aug.last_spans.shape == (1, 2, 2) and set(cf16._aug_plans) == {(24, 32, 20)}
    # the plain call of the same featurizer is untouched by the new cache
    assert torch.equal(cf(samples[1]["frames"][:4]), plain_v[1, : want[1][0].shape[0]]) and set(cf._plans) == {(24, 32)}
    with pytest.raises(ValueError, match="needs a seed"):
        device_collate(samples, lm, cf, video_augment=aug)
    with pytest.raises(ValueError, match="resize = 12 is below the image size 16"):
        VideoAugment(resize=12).frames(cf, samples[0]["frames"], 0, 1)
    for bad, word in ((dict(flip_prob=1.5), "flip_prob"), (dict(time_masks=17), "time_masks"), (dict(time_width=-1), "time_width"),
                      (dict(time_ratio=2.0), "time_ratio"), (dict(resize=0), "resize")):
        with pytest.raises(ValueError, match=word):
            VideoAugment(**bad)


def test_pixels_is_the_in_place_rule(dev):
    from avllm.preprocess import VideoAugment
    g = torch.Generator().manual_seed(3)
    video = torch.randn(3, 5, 3, IMAGE, IMAGE, generator=g)
    aug = VideoAugment(flip_prob=0.5, time_masks=2, time_width=2, time_ratio=0.75, fill=-1.75)
    nframes = torch.tensor([5, 2, 4], dtype=torch.int32, device=dev)
    on_dev = video.to(dev)
    assert aug.pixels(on_dev, nframes, seed=4, first_clip=2) is on_dev
    want, draws = RV.pixels_augment(video.numpy(), [5, 2, 4], 4, first_clip=2, p_flip=0.5, n_time=2, time_width=2, time_ratio=0.75, fill=np.float32(-1.75))
    assert np.array_equal(on_dev.cpu().numpy().view(np.uint32), want.view(np.uint32))
    f = VideoAugment.info_fields(aug.last_info)
    assert f["left"] == f["top"] == [-1, -1, -1] and f["flip"] == [d["flip"] for d in draws] and f["masked"] == [d["masked"] for d in draws]
    null = VideoAugment(flip_prob=0.0)
    same = video.to(dev)
    null.pixels(same, seed=4)
    assert torch.equal(same.cpu(), video) and null.last_info.tolist() == [[-1, -1, 0, 0]] * 3


def test_trainer_augments_training_batches_only(dev, toy):
    from avllm.data import create_dataloaders
    from avllm.preprocess import VideoAugment
    from avllm.trainer import ClipWhisperTrainer
    root, mp, lp = toy
    oc = Wt.tiny()
    m = make_model(oc, Wt.all_weights(oc, 21, lora_b_std=0.05), "fp32").train()
    image, resize = m.cfg.clip.image, m.cfg.clip.image + 8          # the tiny model's CLIP takes 48 x 48: 24 x 32 frames go to 56 x 74
    dl, _ = create_dataloaders(str(mp), str(lp), str(root), m.tokenizer, batch_size=2, shuffle=False, max_video_length=4)
    mk = lambda aug: ClipWhisperTrainer(m, dl, dl, learning_rate=1e-3, max_epochs=1, total_steps=10, video_augment=aug, augment_seed=9)      # noqa: E731
    t0, t1 = mk(None), mk(VideoAugment(**dict(KW, resize=resize)))
    batch = next(iter(dl))
    # the parent's path: device_collate on the same featurizer classes, nothing else
    from avllm.preprocess import ClipFrames, WhisperLogMel, device_collate
    parent_a, parent_v = device_collate(batch["raw"], WhisperLogMel(dev, n_mels=m.cfg.whisper.n_mels), ClipFrames(dev, image=image))
    a0, v0 = t0._unpack(batch)[:2]
    assert torch.equal(a0, parent_a) and torch.equal(v0, parent_v) and t0.last_video_info is None
    a1, v1 = t1._unpack(batch)[:2]
    assert torch.equal(a1, parent_a) and not torch.equal(v1, parent_v)
    for i, (ref, d) in enumerate(restated(batch["raw"], t1.augment_seed_at(0), resize, image)):
        assert np.array_equal(v1[i, : ref.shape[0]].cpu().numpy().view(np.uint32), ref.view(np.uint32)), i
    info, frames = t1.last_video_info
    flipped, masked = t1.video_shares(info.cpu(), frames)
    assert flipped == float(np.mean([d["flip"] for _, d in restated(batch["raw"], t1.augment_seed_at(0), resize, image)]))
    assert masked == pytest.approx(np.mean([d["masked"] / r.shape[0] for r, d in restated(batch["raw"], t1.augment_seed_at(0), resize, image)]))
    # another step, another draw; validation never augments
    t1.global_step = 1
    assert not torch.equal(t1._unpack(batch)[1], v1)
    m.eval()
    a2, v2 = t1._unpack(batch)[:2]
    assert torch.equal(a2, parent_a) and torch.equal(v2, parent_v)
    m.train()
    # precomputed pixel_values: flip and masks only, on a copy, in train() mode only
    feats = {"audio": None, "video": parent_v.cpu(), "labels": batch["labels"], "prompt": None}
    keep = feats["video"].clone()
    out = t1._unpack(feats)[1]
    want, _ = RV.pixels_augment(keep.numpy(), None, t1.augment_seed_at(1), p_flip=KW["flip_prob"], n_time=2, time_width=2, time_ratio=0.75,
                                fill=np.float32(KW["fill"]))
    assert out.is_cuda and torch.equal(feats["video"], keep) and np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert t0._unpack(feats)[1] is feats["video"]
    m.eval()
    assert t1._unpack(feats)[1] is feats["video"]
    m.train()
    # one augmented step end to end
    t1.global_step = 0
    loss = t1.train_step(*t1._unpack(batch))
    assert np.isfinite(float(loss))


def test_config_keys_and_flags_build_the_object(dev):
    from avllm.preprocess import video_augment_from_config
    assert video_augment_from_config({}) is None and video_augment_from_config({"video_time_masks": 0, "video_flip_prob": 0.0}) is None
    a = video_augment_from_config({"video_resize": 256, "video_flip_prob": 0.5, "video_time_masks": 1, "video_time_width": 10, "video_time_ratio": 0.4})
    assert (a.resize, a.random_crop, a.flip_prob, a.time_masks, a.time_width, a.time_ratio, a.fill) == (256, True, 0.5, 1, 10, 0.4, 0.0)
    b = video_augment_from_config({"video_resize": 240, "video_random_crop": False})
    assert (b.resize, b.random_crop, b.flip_prob, b.time_masks) == (240, False, 0.0, 0)
    assert video_augment_from_config({"video_random_crop": True}) is None and video_augment_from_config({"video_random_crop": "false"}) is None
    assert video_augment_from_config({"video_resize": 240, "video_random_crop": "false"}).random_crop is False
    c = video_augment_from_config({"video_flip_prob": 0.25})
    assert (c.resize, c.random_crop, c.flip_prob) == (None, False, 0.25)
    sys.path.insert(0, os.path.join(ROOT, "scripts", "clip_whisper"))
    import train
    from avllm.config import merged
    args = train.parse_args(["--video_resize", "256", "--video_random_crop", "0", "--video_flip_prob", "0.5", "--video_time_masks", "2",
                             "--video_time_width", "12", "--video_time_ratio", "0.3"])
    cfg = merged(None, {k: getattr(args, k) for k in train.VIDEO_KEYS})
    d = video_augment_from_config(cfg)
    assert (d.resize, d.random_crop, d.flip_prob, d.time_masks, d.time_width, d.time_ratio) == (256, False, 0.5, 2, 12, 0.3)
    assert video_augment_from_config(merged(None, {k: getattr(train.parse_args([]), k) for k in train.VIDEO_KEYS})) is None
    assert video_augment_from_config(merged(os.path.join(ROOT, "configs", "clip_whisper.yaml"), {})) is None      # the entries are comments
