"""Acoustic augmentation above the kernels: NoiseBank, AudioAugment and device_collate(augment=), the trainer's audio_augment (training
batches only, a null augment changes nothing, a seed per step and rank) and decode.py --noise_path / --noise_snr, on the tiny model with toy
files written into a temporary directory and noise from a seeded numpy generator."""
import json
import logging
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import refs64_augment as RA  # noqa: E402
from oracle import weights as Wt  # noqa: E402
from test_data_cpu import make_set, write_wav  # noqa: E402
from test_model_gpu import make_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = dict(time_masks=2, time_width=20, time_ratio=0.5, freq_masks=2, freq_width=9)


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    root = tmp_path_factory.mktemp("toy")
    mp, lp = make_set(root, n=4)
    (root / "test.tsv").write_text(mp.read_text()); (root / "test.wrd").write_text(lp.read_text())
    g = np.random.default_rng(7)
    noise = root / "noise"
    noise.mkdir()
    write_wav(noise / "n0.wav", 0.2 * g.standard_normal(3000))
    write_wav(noise / "n1.wav", 0.2 * g.standard_normal((9000, 2)), channels=2)
    np.save(noise / "n2.npy", (0.2 * g.standard_normal(777)).astype(np.float32))
    (noise / "readme.txt").write_text("not a recording")
    return root, mp, lp, noise


def raw_samples(toy, n=4):
    from avllm.data import AVSRDataset
    from avllm.tokenizer import ByteTokenizer
    root, mp, lp, _ = toy
    ds = AVSRDataset(str(mp), str(lp), str(root), ByteTokenizer(512), max_video_length=4)
    return [ds[i] for i in range(n)]


def test_noise_bank_reads_files_as_the_dataset_does(dev, toy, tmp_path):
    from avllm.data import read_audio
    from avllm.preprocess import NoiseBank
    _, _, _, noise = toy
    bank = NoiseBank(str(noise), dev)
    assert len(bank) == 3 and bank.lengths.tolist() == [3000, 9000, 777] and bank.noise.shape == (3, 9000) and bank.noise.dtype == torch.float32
    stereo, _ = read_audio(str(noise / "n1.wav"))
    assert torch.equal(bank.noise[1].cpu(), torch.from_numpy(stereo.mean(axis=1).astype(np.float32)))
    assert float(bank.noise[0, 3000:].abs().max()) == 0.0 and float(bank.noise[2, 777:].abs().max()) == 0.0
    one = NoiseBank(str(noise / "n2.npy"), dev)
    assert len(one) == 1 and torch.equal(one.noise[0, :777].cpu(), torch.from_numpy(np.load(noise / "n2.npy")))
    arrays = NoiseBank([np.ones(5, np.float32), torch.zeros(9)], dev)
    assert arrays.lengths.tolist() == [5, 9] and arrays.noise.shape == (2, 12)
    write_wav(tmp_path / "slow.wav", np.zeros(100), sr=8000)
    with pytest.raises(ValueError, match="slow.wav.*8000 Hz"):
        NoiseBank(str(tmp_path / "slow.wav"), dev)
    (tmp_path / "nothing").mkdir()
    with pytest.raises(ValueError, match="no .wav"):
        NoiseBank(str(tmp_path / "nothing"), dev)


def test_device_collate_is_the_two_ops_around_the_logmel(dev, toy):
    from avllm.preprocess import AudioAugment, ClipFrames, NoiseBank, WhisperLogMel, device_collate, valid_frames
    samples = raw_samples(toy)
    lm, cf = WhisperLogMel(dev), ClipFrames(dev, image=16)
    bank = NoiseBank(str(toy[3]), dev)
    aug = AudioAugment(noise=bank, snr_db=(0.0, 10.0), noise_prob=0.75, **MASKS)
    audio, video = device_collate(samples, lm, cf, max_video_length=4, augment=aug, seed=5)
    info, spans = aug.last_info.clone(), aug.last_spans.clone()
    # by hand
    by_hand = AudioAugment(noise=bank, snr_db=(0.0, 10.0), noise_prob=0.75, **MASKS)
    wave, lengths = lm.pad_batch([s["wave"] for s in samples], return_lengths=True)
    assert lengths.tolist() == [len(s["wave"]) for s in samples]
    valid = valid_frames(lengths)
    assert valid.dtype == torch.int32 and valid.tolist() == [min(3000, -(-len(s["wave"]) // 160)) for s in samples]
    noisy = by_hand.wave(wave, lengths, 5)
    assert noisy.data_ptr() != wave.data_ptr()
    want = by_hand.features(lm(noisy), valid, 5)
    assert torch.equal(audio, want) and torch.equal(info, by_hand.last_info) and torch.equal(spans, by_hand.last_spans)
    plain_a, plain_v = device_collate(samples, lm, cf, max_video_length=4)
    assert torch.equal(video, plain_v) and not torch.equal(audio, plain_a)
    # the draws are the header's rule: the restatement on the bank's own rows
    rows = [bank.noise[i, :n].cpu().numpy() for i, n in enumerate(bank.lengths.tolist())]
    _, infos = RA.add_noise(wave.cpu().numpy(), lengths.tolist(), rows, 5, 0.75, None, 0.0, 10.0)
    got = AudioAugment.info_fields(info)
    assert got["applied"] == [i["applied"] for i in infos] and got["row"] == [i["row"] for i in infos] and got["offset"] == [i["offset"] for i in infos]
    assert 0 < sum(got["applied"])
    want_spans = [RA.spans(b, 5, v, 80, 3000, 2, 20, 0.5, 2, 9) for b, v in enumerate(valid.tolist())]
    assert spans.tolist() == [[list(x) for x in sp] for sp in want_spans]
    assert float(audio[0, :, want_spans[0][0][0]].abs().max()) == 0.0 or want_spans[0][0][1] == 0        # a masked frame holds the fill
    with pytest.raises(ValueError, match="needs a seed"):
        device_collate(samples, lm, cf, augment=aug)


def test_null_augments_give_todays_tensors(dev, toy):
    from avllm.preprocess import AudioAugment, ClipFrames, NoiseBank, WhisperLogMel, device_collate
    samples = raw_samples(toy)
    lm, cf = WhisperLogMel(dev), ClipFrames(dev, image=16)
    today_a, today_v = lm([s["wave"] for s in samples]), None
    a0, v0 = device_collate(samples, lm, cf, max_video_length=4)
    a1, v1 = device_collate(samples, lm, cf, max_video_length=4, augment=None, seed=None)
    null = AudioAugment(noise=NoiseBank(str(toy[3]), dev), noise_prob=0.0)
    a2, v2 = device_collate(samples, lm, cf, max_video_length=4, augment=null, seed=123)
    a3, _ = device_collate(samples, lm, cf, max_video_length=4, augment=AudioAugment(), seed=123)
    assert torch.equal(a0, today_a) and torch.equal(a1, today_a) and torch.equal(a2, today_a) and torch.equal(a3, today_a)
    assert torch.equal(v0, v1) and torch.equal(v0, v2)
    assert null.last_info[:, 0].tolist() == [0, 0, 0, 0] and null.last_spans is None


def run_epochs(dev, toy, augment, epochs=2):
    from avllm.data import create_dataloaders
    from avllm.trainer import ClipWhisperTrainer
    root, mp, lp, _ = toy
    oc = Wt.tiny()
    m = make_model(oc, Wt.all_weights(oc, 21, lora_b_std=0.05), "fp32").train()
    dl, _ = create_dataloaders(str(mp), str(lp), str(root), m.tokenizer, batch_size=2, shuffle=False, max_video_length=4)
    tr = ClipWhisperTrainer(m, dl, dl, learning_rate=1e-3, max_epochs=epochs, total_steps=10, grad_clip=0.5, audio_augment=augment, augment_seed=9)
    losses, audios, rows = [], [], []
    for _ in range(epochs):
        for batch in dl:
            unpacked = tr._unpack(batch)
            audios.append(unpacked[0].clone())
            rows.append(unpacked[2].numel())
            losses.append(float(tr.train_step(*unpacked)))
    return m, tr, dl, losses, audios, rows


def test_trainer_augments_training_batches_only(dev, toy):
    """A null augment trains what no augment trains: the step's inputs, the parameters and both Adam moments after four steps are equal bit
    for bit, which fixes every later loss too.  The REPORTED loss of a step is not repeatable to the bit in this build, with or without an
    augment: avllm_ce_fwd adds the rows' terms onto loss_sum with float atomics, in arrival order (test_connector_train_gpu.same_loss).  Two
    runs of this test's four steps WITHOUT any augment gave 5.636138916 / 5.636139393 at step 1 and 4.823221207 / 4.823221684 at step 3, one
    float32 ulp apart, and a null augment against none gave the same pattern (5.297101021 / 5.297100544 at step 2).  The loss sequences are
    therefore held to that test's bar for this very sum (bars.atomic_sum_term over at most one add per label position); nothing downstream
    reads loss_sum beyond its finiteness."""
    import bars as Bar
    from avllm.preprocess import AudioAugment, NoiseBank
    bank = NoiseBank(str(toy[3]), dev)
    m0, t0, dl, l0, a0, rows = run_epochs(dev, toy, None)
    m1, t1, _, l1, a1, _ = run_epochs(dev, toy, AudioAugment(noise=bank, noise_prob=0.0))
    print("losses without an augment", [repr(x) for x in l0], "with a null augment", [repr(x) for x in l1])
    assert all(torch.equal(x, y) for x, y in zip(a0, a1))
    assert torch.equal(m0.llm_engine.lora_p, m1.llm_engine.lora_p) and torch.equal(t0.m, t1.m) and torch.equal(t0.v, t1.v)
    assert all(abs(x - y) <= Bar.atomic_sum_term(r, max(abs(x), abs(y))) for x, y, r in zip(l0, l1, rows)), (l0, l1)
    aug = AudioAugment(noise=bank, snr_db=5.0, **MASKS)
    m2, t2, _, l2, a2, _ = run_epochs(dev, toy, aug)
    assert all(not torch.equal(x, y) for x, y in zip(a0, a2)) and not torch.equal(m2.llm_engine.lora_p, m0.llm_engine.lora_p)
    assert not torch.equal(a2[0], a2[2])                                                  # the same clips in the second epoch: another step, another draw
    # validation never augments: eval-mode batches are today's, and _validate() is the value of the trainer without an augment on this model
    m2.eval()
    batch = next(iter(dl))
    assert torch.equal(t2._unpack(batch)[0], a0[0])
    m2.train()
    assert not torch.equal(t2._unpack(batch)[0], a0[0])
    t0.model = m2
    # _validate() is the mean of the batches' reported losses, each a loss_sum of avllm_ce_fwd's float atomics (see above): two evaluations of
    # the same model on the same batches are held to the bar of that sum, which is linear in the total and so carries over to the mean (two
    # runs gave 5.612086534 / 5.612086296 and 5.612086296 / 5.612086058, one float32 ulp apart)
    v2, v0 = t2._validate(), t0._validate()
    print("validation losses", repr(v2), repr(v0), "bar", Bar.atomic_sum_term(max(rows), max(abs(v2), abs(v0))))
    assert abs(v2 - v0) <= Bar.atomic_sum_term(max(rows), max(abs(v2), abs(v0))), (v2, v0)
    # the seed of a step: by value, one per step and rank
    assert t2.augment_seed_at(3, 0) == RA.augment_seed(9, 3, 0) != t2.augment_seed_at(3, 1) == RA.augment_seed(9, 3, 1)
    assert t2.augment_seed_at(4) != t2.augment_seed_at(3) and t2.augment_seed_at(2 ** 20, 5) < 2 ** 32
    share, snr = t2.noise_shares(t2.last_augment_info.cpu())
    assert share == 1.0 and snr == 5.0
    # precomputed features: the SpecAugment half only, on a copy
    feats = {"audio": a0[0].cpu(), "video": None, "labels": batch["labels"], "prompt": None}
    out = t2._unpack(feats)[0]
    assert out.is_cuda and not torch.equal(out.cpu(), feats["audio"]) and torch.equal(feats["audio"], a0[0].cpu())
    assert aug.last_spans.shape == (2, 4, 2) and bool((out == 0).any())
    m2.eval()
    assert t2._unpack(feats)[0] is feats["audio"]


def decode_main(argv):
    sys.path.insert(0, os.path.join(ROOT, "scripts", "clip_whisper"))
    import decode
    root_logger = logging.getLogger()
    saved, level = root_logger.handlers[:], root_logger.level
    try:
        assert decode.main(argv) in (None, 0)
    finally:
        for h in root_logger.handlers[:]:
            if h not in saved:
                h.close()
        root_logger.handlers[:] = saved
        root_logger.setLevel(level)


def test_decode_py_noise_flags(dev, toy, tmp_path):
    root, _, _, noise = toy
    base = ["--test_data", str(root / "test.tsv"), "--test_wrd", str(root / "test.wrd"), "--modality", "both", "--batch_size", "2",
            "--max_new_tokens", "4", "--tiny", "--data_path", str(root), "--seed", "3"]
    runs = {}
    for name, extra in (("plain", []), ("noisy", ["--noise_path", str(noise), "--noise_snr", "0"]),
                        ("none mixed", ["--noise_path", str(noise), "--noise_snr", "0", "--noise_prob", "0"])):
        decode_main(base + ["--output_dir", str(tmp_path / name)] + extra)
        runs[name] = json.load(open(tmp_path / name / "decode_results.json"))
    plain, noisy, unmixed = runs["plain"], runs["noisy"], runs["none mixed"]
    assert not {"noise_path", "noise_snr", "noise_prob", "clips_with_noise"} & set(plain)
    assert (noisy["noise_path"], noisy["noise_snr"], noisy["noise_prob"], noisy["clips_with_noise"], noisy["total_samples"]) == (str(noise), 0.0, 1.0, 4, 4)
    assert unmixed["clips_with_noise"] == 0
    # the flags' path with nothing mixed decodes what the plain run decodes
    assert [r["hypothesis"] for r in unmixed["results"]] == [r["hypothesis"] for r in plain["results"]] and unmixed["overall_wer"] == plain["overall_wer"]
    import decode
    for bad in (["--noise_path", str(noise)], ["--noise_snr", "0"], ["--noise_path", str(noise), "--noise_snr", "0", "--synthetic", "2"]):
        with pytest.raises(SystemExit):
            decode.parse_args(base + bad)
