"""Host side of grad_accum_steps (no GPU): argument checking, the default total_steps, the command-line flag and the YAML key reaching the trainer,
the augmentation counter, and the micro-step seed rule restated against the header's constant."""
import importlib.util
import os
import re
import sys
import types

import pytest
import torch

import refs64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fake_model():
    eng = types.SimpleNamespace(lora_p=torch.zeros(8), lora_g=torch.zeros(8), per_layer=4, cfg=types.SimpleNamespace(layers=2))
    return types.SimpleNamespace(llm_engine=eng)


@pytest.mark.parametrize("bad", [0, -1, 2.0, "2", None, True])
def test_bad_grad_accum_steps_is_a_value_error_that_names_it(bad):
    from avllm.trainer import ClipWhisperTrainer
    with pytest.raises(ValueError, match="grad_accum_steps"):
        ClipWhisperTrainer(fake_model(), grad_accum_steps=bad)


@pytest.mark.parametrize("N,batches,want", [(1, 7, 21), (2, 7, 12), (4, 8, 6), (8, 3, 3)])
def test_default_total_steps_counts_windows(N, batches, want):
    from avllm.trainer import ClipWhisperTrainer
    tr = ClipWhisperTrainer(fake_model(), train_dataloader=[0] * batches, max_epochs=3, grad_accum_steps=N, use_graph=False)
    assert tr.total_steps == want and tr.grad_accum_steps == N and tr.micro_step == 0          # max_epochs * ceil(batches / N)
    assert hasattr(tr, "_window") == (N > 1)
    assert tr.flush() is None                                                                  # nothing pending: nothing happens


def test_augmentation_seed_counts_micro_batches():
    from avllm.trainer import ClipWhisperTrainer
    one = ClipWhisperTrainer(fake_model(), use_graph=False, augment_seed=5)
    tr = ClipWhisperTrainer(fake_model(), grad_accum_steps=3, use_graph=False, augment_seed=5)
    seen = set()
    for step in range(2):
        one.global_step = tr.global_step = step
        assert one._augment_index() == step                                                    # N = 1: today's value
        for micro in range(3):
            tr.micro_step = micro
            assert tr._augment_index() == 3 * step + micro
            seen.add(tr.augment_seed_at(tr._augment_index()))
    assert len(seen) == 6
    # after skipped steps the host count runs ahead of the device's; _sync_step() pulls global_step back and the index stays where it is
    for t, N in ((one, 1), (tr, 3)):
        t.global_step, t.micro_step = 5, 0
        t.state.view(torch.int32)[0] = 3                                                       # two of the five steps were skipped on the device
        before = t._augment_index()
        assert before == 5 * N
        assert t._sync_step() == 3 and t.global_step == 3 and t._augment_index() == before
        t.global_step += 1                                                                     # the next step: the next index, synced or not
        assert t._augment_index() == before + N
        assert t._sync_step() == 3 and t._augment_index() == before + N                        # (as if that step was skipped too)
    tr.global_step, tr.micro_step = 3, 0
    tr.state.view(torch.int32)[0], tr.state.view(torch.int32)[6] = 4, 2                        # mid-window: the device count includes the open window
    tr.micro_step = 2
    before = tr._augment_index()
    assert tr._sync_step() == 3 and tr._augment_index() == before


def test_checkpoint_carries_the_augmentation_index(tmp_path):
    """_meta.json's augment_index is restored by load_checkpoint(); a checkpoint without the entry falls back to global_step * grad_accum_steps."""
    import json
    from avllm.trainer import ClipWhisperTrainer
    path = str(tmp_path / "ck.pt")
    json.dump({"global_step": 4, "augment_index": 17, "skipped_steps": 2}, open(path.replace(".pt", "_meta.json"), "w"))
    assert ClipWhisperTrainer.checkpoint_augment_index(path) == 17 and ClipWhisperTrainer.checkpoint_skipped_steps(path) == 2
    json.dump({"global_step": 4}, open(path.replace(".pt", "_meta.json"), "w"))
    assert ClipWhisperTrainer.checkpoint_augment_index(path) is None and ClipWhisperTrainer.checkpoint_skipped_steps(path) is None
    assert ClipWhisperTrainer.checkpoint_augment_index(str(tmp_path / "absent.pt")) is None
    assert ClipWhisperTrainer.checkpoint_skipped_steps(str(tmp_path / "absent.pt")) is None


def load_train_script():
    spec = importlib.util.spec_from_file_location("train_script_under_test", os.path.join(ROOT, "scripts", "clip_whisper", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_main(monkeypatch, tmp_path, argv):
    """scripts/clip_whisper/train.py main() with the model and the trainer replaced by recorders."""
    import avllm.model
    import avllm.trainer
    seen = {}

    class Model:
        def __init__(self, **kw):
            self.cfg, self.tokenizer = types.SimpleNamespace(), None

    class Trainer:
        def __init__(self, model, dl, vdl, **kw):
            seen.update(kw)

        def train(self):
            return {}
    monkeypatch.setattr(avllm.model, "ClipWhisperModel", Model)
    monkeypatch.setattr(avllm.trainer, "ClipWhisperTrainer", Trainer)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(sys, "argv", ["train.py", "--tiny", "--synthetic", "4", "--output_dir", str(tmp_path / "out"), "--llm_path", "none",
                                      "--whisper_model", "none", "--clip_model", "none"] + argv)
    import logging
    handlers, level = logging.root.handlers[:], logging.root.level          # main() configures the root logger: put it back for the other tests
    try:
        load_train_script().main()
    finally:
        for h in logging.root.handlers[:]:
            if h not in handlers:
                logging.root.removeHandler(h)
                h.close()
        logging.root.setLevel(level)
    return seen


def test_flag_and_yaml_reach_the_trainer(monkeypatch, tmp_path):
    assert run_main(monkeypatch, tmp_path, [])["grad_accum_steps"] == 1                        # configs/clip_whisper.yaml
    assert run_main(monkeypatch, tmp_path, ["--grad_accum_steps", "4"])["grad_accum_steps"] == 4
    cfg = tmp_path / "c.yaml"
    cfg.write_text("training:\n  grad_accum_steps: 3\n")
    assert run_main(monkeypatch, tmp_path, ["--config", str(cfg)])["grad_accum_steps"] == 3
    assert run_main(monkeypatch, tmp_path, ["--config", str(cfg), "--grad_accum_steps", "2"])["grad_accum_steps"] == 2


def micro_seed(step, skipped, micro, rank=0):
    """include/avllm.h, avllm_step_advance_micro: the step's seed (tests/refs64.py) plus micro * AVLLM_MICRO_SEED_STRIDE, mod 2^32."""
    return (R.dropout_seed(step, skipped, rank=rank) + micro * 0xC2B2AE35) & 0xFFFFFFFF


def test_micro_seed_rule_against_the_header():
    from avllm import ops
    hdr = open(os.path.join(ROOT, "include", "avllm.h")).read()
    c = int(re.search(r"#define\s+AVLLM_MICRO_SEED_STRIDE\s+(0x[0-9A-Fa-f]+)u", hdr).group(1), 16)
    assert c == 0xC2B2AE35 == ops.MICRO_SEED_STRIDE and c % 2 == 1 and c < 2 ** 32
    assert micro_seed(5, 1, 0, rank=2) == R.dropout_seed(5, 1, rank=2)                          # micro-step 0 keeps the step's seed
    seeds = {micro_seed(s, 0, m, rank=r) for s in range(1, 40) for m in range(8) for r in range(2)}
    assert len(seeds) == 39 * 8 * 2                                                            # windows, micro-steps and ranks do not collide
    # the seeds a step's layers use are base + 0 .. base + 7 * layers - 1: micro-steps of a window stay clear of each other's ranges
    span = 7 * 80
    bases = sorted(micro_seed(3, 0, m) for m in range(16))
    assert min(b - a for a, b in zip(bases, bases[1:])) > span
