#!/usr/bin/env python3
"""Train entry point with the reference's flag names (scripts/clip_whisper/train.py:33-81); `--synthetic N` replaces the
LRS3 manifests with N seeded synthetic clips (no dataset offline).  Launch one process per GPU with torchrun for DDP."""
import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "audio-visual-llm_amd")):
    sys.path.insert(0, p) if p not in sys.path else None

import torch  # noqa: E402


VIDEO_KEYS = ("video_resize", "video_random_crop", "video_flip_prob", "video_time_masks", "video_time_width", "video_time_ratio")


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--config", default=os.path.join(ROOT, "configs", "clip_whisper.yaml"))
    p.add_argument("--output_dir"); p.add_argument("--data_path"); p.add_argument("--llm_path")
    p.add_argument("--whisper_model"); p.add_argument("--clip_model")
    p.add_argument("--modality", choices=["audio", "video", "both"])
    p.add_argument("--batch_size", type=int); p.add_argument("--max_epochs", type=int)
    p.add_argument("--learning_rate", type=float); p.add_argument("--max_seq_len", type=int)
    p.add_argument("--fp16", action="store_true", default=None); p.add_argument("--use_4bit", action="store_true", default=None)
    p.add_argument("--no_lora", action="store_true"); p.add_argument("--lora_r", type=int); p.add_argument("--lora_alpha", type=int)
    p.add_argument("--connector_type", default=None); p.add_argument("--max_grad_norm", type=float)
    p.add_argument("--train_connectors", action="store_true", default=None,
                   help="train the two modality connectors (encoders stay frozen); YAML key model.train_connectors")
    p.add_argument("--lora_target_modules", default=None,
                   help="modules that get a LoRA adapter: comma-separated names out of q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj, or "
                        "all-linear; default the four attention modules (YAML key model.lora_target_modules; a --resume_from checkpoint's own "
                        "value is used when neither is given)")
    p.add_argument("--modality_dropout_audio", type=float, default=None,
                   help="modality dropout: the probability that a clip of a training batch loses its audio (a draw per clip and step, on the "
                        "device; never both streams); default 0 = off (YAML key model.modality_dropout_audio)")
    p.add_argument("--modality_dropout_video", type=float, default=None,
                   help="the probability that a clip loses its video; the two must add up to at most 1 (YAML key model.modality_dropout_video)")
    p.add_argument("--label_smoothing", type=float, default=None,
                   help="label smoothing of the training loss, in [0, 1): F.cross_entropy(label_smoothing=...) on the device; validation keeps "
                        "the plain cross entropy; default 0 = off (YAML key model.label_smoothing; effect on WER not measured)")
    p.add_argument("--z_loss", type=float, default=None,
                   help="coefficient of the auxiliary z-loss z * logsumexp(logits)^2 per scored token (PaLM uses 1e-4), >= 0; training loss "
                        "only; default 0 = off (YAML key model.z_loss)")
    p.add_argument("--noise_path", default=None,
                   help="acoustic augmentation: a .wav / .npy noise recording or a directory of them (16 kHz); a segment of one is mixed into "
                        "each training clip on the device (YAML key data.noise_path; default none = off; effect on WER not measured)")
    p.add_argument("--noise_snr", default=None, help="the SNR in dB: LO,HI (drawn per clip) or one value; default 0,20 (YAML key data.noise_snr)")
    p.add_argument("--noise_prob", type=float, default=None, help="the share of training clips that get noise; default 1 (YAML key data.noise_prob)")
    p.add_argument("--spec_time_masks", type=int, default=None, help="SpecAugment on the log-mel: time masks per clip; default 0 = off (YAML key data.spec_time_masks)")
    p.add_argument("--spec_time_width", type=int, default=None, help="each time mask covers 0..this many frames (YAML key data.spec_time_width)")
    p.add_argument("--spec_time_ratio", type=float, default=None,
                   help="... and at most this share of the clip's own frames; default 1 (YAML key data.spec_time_ratio)")
    p.add_argument("--spec_freq_masks", type=int, default=None, help="frequency masks per clip; default 0 = off (YAML key data.spec_freq_masks)")
    p.add_argument("--spec_freq_width", type=int, default=None, help="each frequency mask covers 0..this many mel bins (YAML key data.spec_freq_width)")
    p.add_argument("--video_resize", type=int, default=None,
                   help="visual augmentation: resize the frames' shorter edge to this (at least the image size) and cut the image-sized window "
                        "at a corner drawn per clip, on the device (YAML key data.video_resize; default none = off; effect on WER not measured)")
    p.add_argument("--video_random_crop", type=int, choices=[0, 1], default=None,
                   help="1: draw the crop window (the default with --video_resize), 0: the centre crop (YAML key data.video_random_crop)")
    p.add_argument("--video_flip_prob", type=float, default=None, help="the share of training clips mirrored left to right; default 0 = off (YAML key data.video_flip_prob)")
    p.add_argument("--video_time_masks", type=int, default=None, help="spans of frames per clip that are blanked; default 0 = off, at most 16 (YAML key data.video_time_masks)")
    p.add_argument("--video_time_width", type=int, default=None, help="each span covers 0..this many frames (YAML key data.video_time_width)")
    p.add_argument("--video_time_ratio", type=float, default=None,
                   help="... and at most this share of the clip's own frames; default 1 (YAML key data.video_time_ratio)")
    p.add_argument("--grad_accum_steps", type=int, default=None,
                   help="micro-batches per optimizer step: a window of N batches is one step on their concatenation (token-mean loss over the "
                        "whole window, on all ranks); default 1 (YAML key training.grad_accum_steps; effect on WER not measured)")
    p.add_argument("--log_interval", type=int); p.add_argument("--save_every", type=int); p.add_argument("--resume_from")
    p.add_argument("--save_steps", type=int, default=None, help="stored by the trainer and never acted on, as in the reference (clip_whisper_trainer.py:94-102)")
    p.add_argument("--log_param_updates", action="store_true", help="accepted for command-line compatibility; the reference stores it and never reads it (:118)")
    p.add_argument("--seed", type=int); p.add_argument("--synthetic", type=int, default=0, help="train on N synthetic clips")
    p.add_argument("--frames", type=int, default=125); p.add_argument("--tiny", action="store_true")
    p.add_argument("--synthetic-weights", action="store_true",
                   help="seeded random weights + byte tokenizer when the model paths are not local checkpoints (implied by --tiny); "
                        "without it such a path is an error")
    return p.parse_args(argv)


class SyntheticClips(torch.utils.data.Dataset):
    """Batches in the reference's 4-tuple layout (audio, video, texts, labels), simple_dataset.py:455."""
    def __init__(self, n, cfg, frames, tok, seed=0):
        self.n, self.cfg, self.frames, self.tok, self.seed = n, cfg, frames, tok, seed
    def __len__(self):
        return self.n
    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        audio = torch.randn(80, 2 * self.cfg.whisper.n_ctx, generator=g)
        video = torch.randn(self.frames, 3, self.cfg.clip.image, self.cfg.clip.image, generator=g)
        words = " ".join("w%d" % int(x) for x in torch.randint(0, 50, (int(torch.randint(3, 9, (1,), generator=g)),), generator=g))
        ids = self.tok([words], padding="max_length", max_length=256, truncation=True).input_ids[0]
        return audio, video, words, ids
    @staticmethod
    def collate(b):
        return torch.stack([x[0] for x in b]), torch.stack([x[1] for x in b]), [x[2] for x in b], torch.stack([x[3] for x in b])


def main():
    a = parse_args()
    from avllm.config import merged
    cfg = merged(a.config, {"output_dir": a.output_dir, "path": a.data_path, "llm_path": a.llm_path, "whisper_model": a.whisper_model,
                            "clip_model": a.clip_model, "modality": a.modality, "batch_size": a.batch_size, "num_epochs": a.max_epochs,
                            "learning_rate": a.learning_rate, "max_seq_len": a.max_seq_len, "use_fp16": a.fp16, "use_4bit": a.use_4bit,
                            "lora_r": a.lora_r, "lora_alpha": a.lora_alpha, "connector_type": a.connector_type, "train_connectors": a.train_connectors,
                            "lora_target_modules": a.lora_target_modules, "modality_dropout_audio": a.modality_dropout_audio,
                            "modality_dropout_video": a.modality_dropout_video, "label_smoothing": a.label_smoothing, "z_loss": a.z_loss, "max_grad_norm": a.max_grad_norm, "log_interval": a.log_interval, "save_every": a.save_every, "seed": a.seed,
                            "grad_accum_steps": a.grad_accum_steps, "save_steps": a.save_steps, "log_param_updates": a.log_param_updates or None,
                            "noise_path": a.noise_path, "noise_snr": a.noise_snr, "noise_prob": a.noise_prob, "spec_time_masks": a.spec_time_masks,
                            "spec_time_width": a.spec_time_width, "spec_time_ratio": a.spec_time_ratio, "spec_freq_masks": a.spec_freq_masks,
                            "spec_freq_width": a.spec_freq_width, **{k: getattr(a, k) for k in VIDEO_KEYS}})
    os.makedirs(cfg["output_dir"], exist_ok=True)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s",
                        handlers=[logging.StreamHandler(), logging.FileHandler(os.path.join(cfg["output_dir"], "training.log"))])
    world = int(os.environ.get("WORLD_SIZE", "1")); local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        torch.distributed.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"))
    torch.manual_seed(cfg.get("seed", 42))
    from avllm.model import ClipWhisperModel
    from avllm.trainer import ClipWhisperTrainer
    kw = {}
    targets = cfg.get("lora_target_modules")
    if targets is None and a.resume_from and not a.no_lora:
        targets = ClipWhisperTrainer.checkpoint_lora_targets(a.resume_from)      # a resume trains the modules the checkpoint holds
    if targets is not None:
        kw["lora_target_modules"] = targets
    if a.tiny:
        from avllm.arch import ClipCfg, LlamaCfg, LoraCfg, ModelCfg, WhisperCfg
        kw["config"] = ModelCfg(WhisperCfg(128, 2, 2, 256), ClipCfg(128, 2, 2, 256, 48, 16), LlamaCfg(256, 2, 2, 512, 512), LoraCfg(16, 32.0))
    model = ClipWhisperModel(llm_path=cfg["llm_path"], whisper_model=cfg["whisper_model"], clip_model=cfg["clip_model"], device=f"cuda:{local}",
                             use_fp16=bool(cfg.get("use_fp16")), use_4bit=bool(cfg.get("use_4bit")), use_lora=not a.no_lora,
                             lora_r=cfg.get("lora_r", 16), lora_alpha=cfg.get("lora_alpha", 32), lora_dropout=cfg.get("lora_dropout", 0.05),
                             freeze_encoders=cfg.get("freeze_encoders", True), modality=cfg.get("modality", "both"),
                             max_seq_len=cfg.get("max_seq_len", 256), fusion_scale=cfg.get("fusion_scale", 0.5),
                             connector_type=cfg.get("connector_type", "simple"), train_connectors=bool(cfg.get("train_connectors", False)),
                             modality_dropout_audio=float(cfg.get("modality_dropout_audio") or 0.0),
                             modality_dropout_video=float(cfg.get("modality_dropout_video") or 0.0),
                             label_smoothing=float(cfg.get("label_smoothing") or 0.0), z_loss=float(cfg.get("z_loss") or 0.0),
                             synthetic_weights=a.synthetic_weights or a.tiny, **kw)
    if a.synthetic:
        frames = a.frames if not a.tiny else 5
        ds = SyntheticClips(a.synthetic, model.cfg, frames, model.tokenizer, cfg.get("seed", 42))
        sampler = torch.utils.data.distributed.DistributedSampler(ds, shuffle=True) if world > 1 else None
        dl = torch.utils.data.DataLoader(ds, batch_size=cfg.get("batch_size", 4), shuffle=sampler is None, sampler=sampler, collate_fn=ds.collate)
        vdl = torch.utils.data.DataLoader(SyntheticClips(max(2, a.synthetic // 8), model.cfg, frames, model.tokenizer, 7), batch_size=cfg.get("batch_size", 4), collate_fn=ds.collate)
    else:
        # LRS3-style manifests (configs/clip_whisper.yaml data.path / train_manifest / train_labels): raw samples, features on the device
        from avllm.data import AVSRDataset, create_dataloaders
        root = cfg.get("path") or "."
        mp = os.path.join(root, cfg.get("train_manifest", "train.tsv")); lp = os.path.join(root, cfg.get("train_labels", "train.wrd"))
        sampler = None
        if world > 1:
            sampler = torch.utils.data.distributed.DistributedSampler(AVSRDataset(mp, lp, root, model.tokenizer, modality=cfg.get("modality", "both")), shuffle=True)
        dl, vdl = create_dataloaders(mp, lp, root, model.tokenizer, batch_size=cfg.get("batch_size", 4), num_workers=cfg.get("num_workers", 0),
                                     modality=cfg.get("modality", "both"), max_video_length=cfg.get("max_video_length", 300), sampler=sampler)
    from avllm.preprocess import augment_from_config, video_augment_from_config
    augment = augment_from_config(cfg, f"cuda:{local}")
    tr = ClipWhisperTrainer(model, dl, vdl, audio_augment=augment, video_augment=video_augment_from_config(cfg), augment_seed=cfg.get("seed", 42), learning_rate=float(cfg.get("learning_rate", 5e-5)), weight_decay=float(cfg.get("weight_decay", 0.01)),
                            max_epochs=cfg.get("num_epochs", 10), output_dir=cfg["output_dir"], device=f"cuda:{local}", fp16=bool(cfg.get("use_fp16")),
                            grad_accum_steps=cfg.get("grad_accum_steps", 1), log_interval=cfg.get("log_interval", 10), save_every=cfg.get("save_every", 1),
                            grad_clip=float(cfg.get("max_grad_norm", 0.5)), warmup_steps=cfg.get("warmup_steps", 0),
                            save_steps=cfg.get("save_steps", None), log_param_updates=bool(cfg.get("log_param_updates", False)))
    if a.resume_from:
        tr.load_checkpoint(a.resume_from)
    print(tr.train())


if __name__ == "__main__":
    main()
