"""ClipWhisperTrainer -- mirror of src/clip_whisper/trainer/clip_whisper_trainer.py:19-1017 for the hot loop
(`_train_epoch` :412-524, `_process_batch` :604-723, `_setup_optimizer` :171-232, `_validate` :526-603) with the
same constructor keywords, batch layouts, return dict and output files.  The step is:
  encoders (HIP) -> fuse/pool (HIP) -> Llama+LoRA fwd+loss (HIP) -> bwd (HIP) [-> RCCL all-reduce, overlapped]
  -> clip_grad_norm_ + AdamW fused on the flat LoRA buffer (HIP) -> cosine LR.
With a model built with train_connectors=True the backward pass also leaves d(inputs_embeds), the fusion / pooling adjoint and the two weight
gradients fill the flat connector gradient (one sequential chain after the piece that ends at layer 0), and ONE clip + ONE AdamW step cover
the LoRA buffer and the connector buffer together (weights decayed, biases not: _setup_optimizer :183-197).
No `loss.item()` inside the step: the loss stays on the device and is read once per log interval.

The step is graph-replayable: everything that changes from step to step (learning rate, Adam's bias corrections, the LoRA dropout
seed) lives in a small device record advanced by a one-thread kernel at the top of the step (include/avllm.h avllm_step_state), so the
~1,400 kernel launches of a step are the same sequence every time.  With `use_graph` (default on) the step is captured once per input
signature into hipGraphs (torch.cuda.CUDAGraph owns capture + memory pool) and replayed: one graph when single-process; under data
parallelism forward / backward pieces / optimizer are separate graphs with the RCCL collectives issued between them, each backward
piece's gradient all-reduce running on the side stream under the next piece.

grad_accum_steps = N > 1: a window of N calls of train_step() is ONE optimizer step on the concatenation of their micro-batches (token-mean loss
over all scored tokens of the window on all ranks).  Micro-steps back-propagate the sum cross entropy and add into the gradient buffers; the
closing part divides by the window's count on the device (DESIGN.md §4 "Gradient accumulation").  N = 1 is the step described above.
"""
from __future__ import annotations

import csv
import ctypes
import json
import logging
import math
import os
import time

import torch

from . import lib as L
from . import ops
from .dist import LoraGradReducer, is_dist
from .engine import Workspace


class ClipWhisperTrainer:
    def __init__(self, model, train_dataloader=None, val_dataloader=None, learning_rate=5e-5, weight_decay=0.01, max_epochs=10,
                 output_dir="outputs/clip_whisper", device="cuda", fp16=False, grad_accum_steps=1, log_interval=10, save_every=1,
                 save_steps=None, grad_clip=0.5, warmup_steps=0, log_param_updates=False, total_steps=None, use_graph=None,
                 bwd_pieces=None, audio_augment=None, augment_seed=0, video_augment=None):
        self.model, self.train_dataloader, self.val_dataloader = model, train_dataloader, val_dataloader
        # acoustic augmentation (avllm.preprocess.AudioAugment | None): applied in _unpack, in front of the captured step, in train() mode only
        self.audio_augment, self.augment_seed = audio_augment, int(augment_seed)
        self.last_augment_info = None                      # AudioAugment.last_info of the last augmented batch (device int32 [B, 5])
        self._augment_notes = set()
        # visual augmentation (avllm.preprocess.VideoAugment | None): in _unpack too, train() mode only, the same step seed under another salt
        self.video_augment = video_augment
        self.last_video_info = None                        # (VideoAugment.last_info, the clips' frame counts) of the last augmented batch
        self.learning_rate, self.weight_decay, self.max_epochs = learning_rate, weight_decay, max_epochs
        self.output_dir, self.device, self.fp16 = output_dir, device, fp16
        # N micro-batches per optimizer step: a window of N calls of train_step() is ONE step on their concatenation (the reference stores the
        # keyword and never reads it).  1 = every call is an optimizer step.
        if isinstance(grad_accum_steps, bool) or not isinstance(grad_accum_steps, int) or grad_accum_steps < 1:
            raise ValueError(f"grad_accum_steps must be an int >= 1, got {grad_accum_steps!r}")
        self.grad_accum_steps = grad_accum_steps
        self.micro_step = 0                                # micro-batches of the open window (host side; 0 .. N-1)
        self._augment_skew = 0                             # micro-batches of skipped windows that _sync_step() took out of global_step (_augment_index)
        self.log_interval, self.save_every, self.save_steps = log_interval, max(1, save_every or 1), save_steps
        self.grad_clip, self.warmup_steps = grad_clip, warmup_steps
        self.global_step = 0
        self.train_losses, self.val_losses, self.best_val_loss = [], [], float("inf")
        if total_steps is None:                            # optimizer steps: a partial last window of an epoch is one (flush())
            total_steps = max_epochs * (-(-len(train_dataloader) // grad_accum_steps) if train_dataloader is not None else 1)
        self.total_steps = max(1, total_steps)
        eng = model.llm_engine
        self.m = torch.zeros_like(eng.lora_p)
        self.v = torch.zeros_like(eng.lora_p)
        self.sumsq = torch.zeros(1, device=eng.lora_p.device, dtype=torch.float32)
        self._sumsq_parts = torch.zeros(1024, device=eng.lora_p.device, dtype=torch.float32)      # fixed-order gradient norm: replicas stay bit-identical
        self.skipped = torch.zeros(1, device=eng.lora_p.device, dtype=torch.float32)      # optimizer steps skipped on a non-finite loss / gradient
        self.reducer = LoraGradReducer(eng.lora_g, eng.per_layer, eng.cfg.layers)
        dev = eng.lora_p.device
        # train_connectors=True: the connectors' Adam moments, flat like model.conn_p / model.conn_g (audio W, audio b, video W, video b)
        self.train_connectors = bool(getattr(model, "train_connectors", False))
        if self.train_connectors:
            self.cm = torch.zeros_like(model.conn_p)
            self.cv = torch.zeros_like(model.conn_p)
        # avllm_step_state on the device: step count, this step's lr / bias corrections / dropout seed
        self.state = torch.zeros(ctypes.sizeof(L.StepState), dtype=torch.uint8, device=dev)
        self._seed_ptr = self.state.data_ptr() + L.StepState.dropout_seed.offset
        self._loss_buf = torch.zeros((), dtype=torch.float32, device=dev)
        # label smoothing / z-loss (model.label_smoothing, model.z_loss): train_step() returns the composite objective; last_nll holds this
        # rank's mean plain cross entropy of the last (micro-)batch, a device scalar written inside the (captured) step; None with both off
        self.label_smoothing, self.z_loss = float(getattr(model, "label_smoothing", 0.0)), float(getattr(model, "z_loss", 0.0))
        self.last_nll = torch.zeros((), dtype=torch.float32, device=dev) if (self.label_smoothing or self.z_loss) else None
        self._rank = torch.distributed.get_rank() if is_dist() else 0
        if use_graph is None:
            use_graph = os.environ.get("AVLLM_GRAPH", "1") != "0"
        self.use_graph = bool(use_graph) and dev.type == "cuda"
        # data parallel + graphs: the backward pass is replayed in pieces so that a piece's gradient all-reduce overlaps the next piece
        self.bwd_pieces = max(1, min(eng.cfg.layers, bwd_pieces if bwd_pieces is not None else (4 if is_dist() else 1)))
        self._graphs = {}
        if grad_accum_steps > 1:
            # the window's [loss_sum, count] (avllm_window_add), the divisor 1.0 every micro-step back-propagates the SUM cross entropy with,
            # this rank's mean loss of the last micro-batch and the global token-mean of the last closed window
            self._window = torch.zeros(2, dtype=torch.float32, device=dev)
            self._one = torch.ones(1, dtype=torch.float32, device=dev)
            self._micro_loss = torch.zeros((), dtype=torch.float32, device=dev)
            self.window_loss = torch.zeros((), dtype=torch.float32, device=dev)
            self._close_graph = None                       # None -> "warm" -> captured, as a signature's graphs
            self._deferred_save = None                     # a checkpoint asked for mid-window, written when the window closes

    # ---- _setup_optimizer :171-232: AdamW(beta 0.9/0.95, eps 1e-8); cosine (with optional linear warmup)
    def lr_at(self, step):
        if self.warmup_steps > 0:
            if step < self.warmup_steps:
                return self.learning_rate * step / max(1, self.warmup_steps)
            prog = (step - self.warmup_steps) / max(1, self.total_steps - self.warmup_steps)
            return self.learning_rate * max(0.0, 0.5 * (1.0 + math.cos(math.pi * prog)))
        return self.learning_rate * (1 + math.cos(math.pi * step / self.total_steps)) / 2

    def augment_seed_at(self, step, rank=None):
        """The seed of the augmentation draws for micro-batch number `step` (the count of micro-batches before it, _augment_index(); with
        grad_accum_steps = 1 the count of optimizer steps taken before it) on `rank`: by value, so every rank and every micro-batch draws
        its own noise and masks, and a run repeats."""
        return (self.augment_seed + 1000003 * int(step) + 7919 * (self._rank if rank is None else int(rank))) & 0xFFFFFFFF

    def _augment_index(self):
        """The number of the micro-batch about to be unpacked: grad_accum_steps * the windows closed so far, skipped ones included, + the open
        window's micro-steps, so the micro-batches of a window are not given the same noise and masks.  The count is the host's own: when
        _sync_step() takes the skipped steps out of global_step it adds them to _augment_skew, so the index does not move there and the
        draws of a run do not depend on log_interval or on when a checkpoint was written.  _save_checkpoint() writes it into `_meta.json`."""
        return self.global_step * self.grad_accum_steps + self.micro_step + self._augment_skew

    def _augment_features(self, audio):
        """A batch of precomputed features has no waveform to mix noise into: it gets the SpecAugment half only, every frame counted as
        valid, on a device copy (the loader's tensor is left as it is)."""
        aug = self.audio_augment
        if aug is None or not self.model.training or audio is None or not aug.masks:
            return audio
        if "features" not in self._augment_notes:
            self._augment_notes.add("features")
            logging.info("audio_augment on precomputed features: SpecAugment only (valid = all frames); noise needs raw waveforms")
        audio = audio.to(self.model.device, torch.float32, copy=True).contiguous()
        return aug.features(audio, None, self.augment_seed_at(self._augment_index()))

    def _augment_pixels(self, video):
        """A batch of precomputed pixel_values [B, F, 3, S, S] was resized and cropped by whoever made it: it gets the flip and the frame masks
        only, every frame counted as the clip's own, on a device copy (the loader's tensor is left as it is)."""
        aug = self.video_augment
        if aug is None or not self.model.training or video is None or video.dim() != 5:
            return video
        if "pixels" not in self._augment_notes:
            self._augment_notes.add("pixels")
            logging.info("video_augment on precomputed pixel_values: flip and frame masks only (all frames counted); the crop needs raw frames")
        dtype = video.dtype if video.dtype in (torch.float32, torch.bfloat16) else torch.float32      # the kernel moves fp32 or bf16 cells
        video = video.to(self.model.device, dtype, copy=True).contiguous()
        aug.pixels(video, None, self.augment_seed_at(self._augment_index()))
        self.last_video_info = (aug.last_info, aug.last_frames)
        return video

    # ---- _process_batch :604-680
    def _unpack(self, batch):
        if isinstance(batch, dict) and "raw" in batch:
            # raw samples from avllm.data.AVSRDataset: log-mel / layer norm / CLIP resize+normalise happen here, on the device
            from .preprocess import ClipFrames, WhisperLogMel, device_collate
            if getattr(self, "_featurizers", None) is None:
                dev = self.model.device
                self._featurizers = (WhisperLogMel(dev, n_mels=self.model.cfg.whisper.n_mels), ClipFrames(dev, image=self.model.cfg.clip.image))
            if (self.audio_augment is not None or self.video_augment is not None) and self.model.training:
                audio, video = device_collate(batch["raw"], *self._featurizers, augment=self.audio_augment,
                                              seed=self.augment_seed_at(self._augment_index()), video_augment=self.video_augment)
                if audio is not None and self.audio_augment is not None and self.audio_augment.mixes:
                    self.last_augment_info = self.audio_augment.last_info
                if video is not None and self.video_augment is not None:
                    self.last_video_info = (self.video_augment.last_info, self.video_augment.last_frames)
            else:
                audio, video = device_collate(batch["raw"], *self._featurizers)
            tok = self.model.tokenizer(batch["texts"], return_tensors="pt", padding=True, truncation=True, max_length=self.model.max_seq_len)
            return audio, video, batch["labels"], tok.input_ids
        if isinstance(batch, dict):
            return self._augment_features(batch.get("audio")), self._augment_pixels(batch.get("video")), batch.get("labels"), batch.get("prompt")
        audio, video, texts, labels = batch
        audio, video = self._augment_features(audio), self._augment_pixels(video)
        tok = self.model.tokenizer(texts, return_tensors="pt", padding=True, truncation=True, max_length=self.model.max_seq_len)
        bs = labels.shape[0]
        for t in (audio, video):
            if t is not None and t.shape[0] != bs:
                raise AssertionError(f"Batch size mismatch: {t.shape[0]} vs labels {bs}")
        return audio, video, labels, tok.input_ids

    # ---- the step, in capture-safe parts (no host sync, no host-side per-step scalars)
    def _part_fwd(self, audio, video, labels, prompt):
        model, eng = self.model, self.model.llm_engine
        ops.step_advance(self.state, self.learning_rate, self.total_steps, self.warmup_steps, rank=self._rank)
        labels = model._prep_labels(labels)
        # modality dropout (model.modality_dropout_*): drawn here, after step_advance, from this step's seed in device memory -- a replayed
        # graph redraws
        x = model._llm_inputs(audio, video, prompt, S_out=labels.shape[1], keep=self.train_connectors, seed_dev=self._seed_ptr)
        p = float(model.lora_dropout) if (model.training and model.use_lora and model.lora_dropout) else 0.0
        eng.fwd_loss(x, labels, dropout=p, seed=0, seed_dev=self._seed_ptr, label_smoothing=self.label_smoothing, z_loss=self.z_loss)
        if self.last_nll is not None:
            torch.div(eng.loss_terms[0], eng.acc[1], out=self.last_nll)

    def _piece_range(self, i):
        """Decoder layers (hi, lo) of backward piece i of self.bwd_pieces, last layer first."""
        n, k = self.model.llm_engine.cfg.layers, self.bwd_pieces
        hi = n - 1 - (i * n) // k
        lo = n - ((i + 1) * n) // k
        return hi, lo

    def _part_bwd(self, i, per_layer_cb=None):
        eng = self.model.llm_engine
        if i == 0:
            eng.lora_g.zero_()
        hi, lo = self._piece_range(i)
        if self.train_connectors and lo == 0:
            # the piece that ends at layer 0 also leaves d(inputs_embeds); the connector backward follows it on the same stream
            eng.bwd(grad_scale=1.0, count=eng.acc[1:2], after_layer=per_layer_cb, layer_hi=hi, layer_lo=lo, dx_embeds=self.model._dx_embeds_buffer())
            self.model.connector_backward()
            return
        eng.bwd(grad_scale=1.0, count=eng.acc[1:2], after_layer=per_layer_cb, layer_hi=hi, layer_lo=lo)

    def _connector_segments(self):
        """(p, g, m, v, weight_decay) per connector tensor: weights decay, biases do not (_setup_optimizer :183-197)."""
        m = self.model
        return [(m.conn_p[a:b], m.conn_g[a:b], self.cm[a:b], self.cv[a:b], self.weight_decay if len(shape) == 2 else 0.0)
                for a, b, shape in m.conn_slices]

    def _part_opt_connectors(self):
        """clip_grad_norm_(model.parameters()) is ONE global norm over connector and LoRA gradients (trainer :457-460), formed in a fixed
        order; the update of every buffer is ONE launch under one guard decision, so a non-finite step is skipped -- and counted, and the
        step count taken back -- exactly once, with no buffer touched."""
        eng = self.model.llm_engine
        ops.grad_sumsq_multi([self.model.conn_g, eng.lora_g], self.sumsq, self._sumsq_parts)
        segs = self._connector_segments() + [(eng.lora_p, eng.lora_g, self.m, self.v, self.weight_decay)]
        ops.adamw_step_multi(segs, 0.0, 0, sumsq=self.sumsq, max_norm=self.grad_clip or 0.0, guard=eng.acc[0:1], skipped=self.skipped,
                             state=self.state)
        eng.pack_lora()
        self.model.refresh_connectors()
        torch.div(eng.acc[0], eng.acc[1], out=self._loss_buf)

    def _part_opt(self):
        eng = self.model.llm_engine
        if self.train_connectors:
            return self._part_opt_connectors()
        ops.grad_sumsq(eng.lora_g, self.sumsq, partials=self._sumsq_parts)
        # NaN/Inf guard of trainer :444-452 without a host sync: a non-finite (all-reduced) loss sum or gradient norm makes the update a
        # no-op on every rank alike (the all-reduce spreads the NaN), leaving lora_p, m and v untouched; `skipped_steps` counts them and
        # the device-side step count goes back by one, so neither the LR schedule nor Adam's bias corrections advance (as in the reference,
        # which runs neither optimizer.step() nor scheduler.step() on such a batch).
        ops.adamw_step(eng.lora_p, eng.lora_g, self.m, self.v, 0.0, 0, sumsq=self.sumsq, max_norm=self.grad_clip or 0.0, wd=self.weight_decay,
                       guard=eng.acc[0:1], skipped=self.skipped, state=self.state)
        eng.pack_lora()
        torch.div(eng.acc[0], eng.acc[1], out=self._loss_buf)

    # ---- grad_accum_steps > 1: the micro-step (forward, backward, accumulate) and the part that closes a window.  Neither depends on the
    # micro-step's number: what differs between micro-steps is read from device memory (avllm_step_advance_micro, avllm_window_add), so ONE
    # capture per input signature serves every position in a window and a window may mix signatures.
    def _part_micro_fwd(self, audio, video, labels, prompt):
        model, eng = self.model, self.model.llm_engine
        ops.step_advance_micro(self.state, self.learning_rate, self.total_steps, self.warmup_steps, rank=self._rank)
        labels = model._prep_labels(labels)
        x = model._llm_inputs(audio, video, prompt, S_out=labels.shape[1], keep=self.train_connectors, seed_dev=self._seed_ptr)
        p = float(model.lora_dropout) if (model.training and model.use_lora and model.lora_dropout) else 0.0
        eng.fwd_loss(x, labels, dropout=p, seed=0, seed_dev=self._seed_ptr, label_smoothing=self.label_smoothing, z_loss=self.z_loss)
        if self.last_nll is not None:
            torch.div(eng.loss_terms[0], eng.acc[1], out=self.last_nll)
        ops.window_add(self._window, eng.acc, self.state)
        torch.div(eng.acc[0], eng.acc[1], out=self._micro_loss)

    def _part_micro_bwd(self, i):
        """Backward piece i of the SUM cross entropy (divisor 1.0, grad_scale 1): lora_g and conn_g are added to, never zeroed here."""
        eng = self.model.llm_engine
        hi, lo = self._piece_range(i)
        if self.train_connectors and lo == 0:
            eng.bwd(grad_scale=1.0, count=self._one, layer_hi=hi, layer_lo=lo, dx_embeds=self.model._dx_embeds_buffer())
            self.model.connector_backward(accumulate=True)
            return
        eng.bwd(grad_scale=1.0, count=self._one, layer_hi=hi, layer_lo=lo)

    def _part_close(self):
        """One global norm over the window's gradient, one clip, one guard decision, one AdamW step: the gradient buffers hold SUMS over the
        window's scored tokens and the optimizer divides by their (all-reduced) count, read from device memory.  The guard is the window's
        loss sum: a non-finite value anywhere in the window skips the window once."""
        eng = self.model.llm_engine
        count, guard = self._window[1:2], self._window[0:1]
        if self.train_connectors:
            ops.grad_sumsq_multi([self.model.conn_g, eng.lora_g], self.sumsq, self._sumsq_parts)
            segs = self._connector_segments() + [(eng.lora_p, eng.lora_g, self.m, self.v, self.weight_decay)]
            ops.adamw_step_multi(segs, 0.0, 0, sumsq=self.sumsq, max_norm=self.grad_clip or 0.0, guard=guard, skipped=self.skipped,
                                 state=self.state, grad_div=count)
            eng.pack_lora()
            self.model.refresh_connectors()
        else:
            ops.grad_sumsq(eng.lora_g, self.sumsq, partials=self._sumsq_parts)
            ops.adamw_step(eng.lora_p, eng.lora_g, self.m, self.v, 0.0, 0, sumsq=self.sumsq, max_norm=self.grad_clip or 0.0, wd=self.weight_decay,
                           guard=guard, skipped=self.skipped, state=self.state, grad_div=count)
            eng.pack_lora()
        torch.div(self._window[0], self._window[1], out=self.window_loss)

    def _eager_micro(self, audio, video, labels, prompt, closing):
        """The micro-step's launches; only the closing one issues collectives, one all-reduce per backward piece as in _eager_step, whether
        graphs are on or off (a rank in eager and a rank in replay issue the same ones in the same order)."""
        self._part_micro_fwd(audio, video, labels, prompt)
        for i in range(self.bwd_pieces):
            self._part_micro_bwd(i)
            if closing:
                hi, lo = self._piece_range(i)
                self.reducer.layers_done(lo, hi)

    def _replay_micro(self, st, closing):
        if "all" in st:
            st["all"].replay()
            return
        st["fwd"].replay()
        for i, g in enumerate(st["bwd"]):
            g.replay()
            if closing:
                hi, lo = self._piece_range(i)
                self.reducer.layers_done(lo, hi)

    def _close_window(self, use_graph, reduce_all=False):
        """The rest of the window's collectives (the connector bucket, then the window's [loss_sum, count] once; reduce_all: a partial window
        closed by flush() has not all-reduced its LoRA gradient piece by piece), then the closing part, warm -> capture -> replay."""
        eng = self.model.llm_engine
        if reduce_all:
            self.reducer.bucket_done(eng.lora_g)
        if self.train_connectors:
            self.reducer.bucket_done(self.model.conn_g)
        self.reducer.finish()
        self.reducer.reduce_counts(self._window)
        g = self._close_graph if use_graph else None
        if use_graph:
            if isinstance(g, tuple) and g[1] != Workspace.generation:
                self._close_graph = g = None
            if g is None:
                self._close_graph = "warm"
            elif g == "warm":
                graph = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(graph, pool=torch.cuda.graph_pool_handle()):
                    self._part_close()
                self._close_graph = g = (graph, Workspace.generation)
        if isinstance(g, tuple):
            g[0].replay()
        else:
            self._part_close()
        self.micro_step = 0
        self.global_step += 1
        if self._deferred_save is not None:
            args, self._deferred_save = self._deferred_save, None
            self._save_checkpoint(*args)

    def _abandon_window(self):
        """A micro-step raised half way (single process only): its launches may have added part of a gradient, so the open window is given
        up -- the step its first advance started is taken back, the next call opens a new window that zeroes the sums.  One host sync, on an
        error path.
        Single process only: under data parallelism _train_epoch re-raises instead (the other ranks are inside the collectives), and nothing
        here is agreed between ranks.  It assumes the window's closing launch has NOT run: that launch resets the micro-step count itself and,
        on a skipped window, has already taken the step back; with the count at 0 this function therefore leaves the device state alone, and
        it must not be called on a window that has closed."""
        words = self.state.view(torch.int32)
        if int(words[6]) > 0:
            words[0] -= 1
            words[6] = 0
        dropped, self.micro_step = self.micro_step, 0
        return dropped

    def flush(self):
        """Close a partial window: one optimizer step on the micro-batches accumulated so far.  Does nothing (and returns None) when nothing
        is pending; otherwise returns the window's loss.  Under data parallelism every rank must call it at the same point."""
        if self.grad_accum_steps == 1 or self.micro_step == 0:
            return None
        self._close_window(self.use_graph, reduce_all=True)
        return self.window_loss.clone()

    def window_gradients(self):
        """{"lora_g": ..., "conn_g": ... (None unless the connectors train)}: clones of the gradient of the last closed window's loss -- the
        token-mean cross entropy over all its scored tokens on all ranks -- before clipping.
        With grad_accum_steps > 1 the raw buffers (llm_engine.lora_g, model.conn_g) hold something else: the SUM over the window's scored
        tokens of the per-token gradients, on this rank until the closing micro-step's all-reduce and over all ranks after it; the optimizer
        divides by the window's count on the fly and never writes the quotient back.  They hold it from the closing micro-step (or flush())
        until the first micro-step of the next window zeroes them; in between -- mid-window -- they hold that window's partial sums and this
        method's result is not a gradient of anything.  With grad_accum_steps = 1 the buffers hold the batch's mean gradient itself."""
        eng = self.model.llm_engine
        gs = {"lora_g": eng.lora_g.clone(), "conn_g": self.model.conn_g.clone() if self.train_connectors else None}
        if self.grad_accum_steps > 1:
            inv = torch.where(self._window[1] > 0, 1.0 / self._window[1], torch.zeros_like(self._window[1]))
            for g in gs.values():
                if g is not None:
                    g.mul_(inv)
        return gs

    def _micro_train_step(self, audio, video, labels, prompt, use_graph):
        """train_step() with grad_accum_steps = N > 1: one micro-step; the N-th closes the window."""
        eng = self.model.llm_engine
        closing = self.micro_step == self.grad_accum_steps - 1
        if self.micro_step == 0:                         # a new window: the gradient sums start from zero (the temporaries da / dv / dx_embeds
            eng.lora_g.zero_()                           # are per micro-step anyway)
            if self.train_connectors:
                self.model.conn_g.zero_()
        st = self._graph_state(audio, video, labels, prompt, micro=True) if use_graph else None
        if isinstance(st, dict):
            for dst, src in zip(st["inputs"], (audio, video, labels, prompt)):
                if dst is not None and src.data_ptr() != dst.data_ptr():
                    dst.copy_(src, non_blocking=True)
            self._replay_micro(st, closing)
            self.model.last_modality_modes = st["modes"]
        else:
            self._eager_micro(audio, video, labels, prompt, closing)
        loss = self._micro_loss.clone()
        self.micro_step += 1
        if closing:
            self._close_window(use_graph)
        return loss

    def _eager_step(self, audio, video, labels, prompt):
        eng = self.model.llm_engine
        self._part_fwd(audio, video, labels, prompt)
        self.reducer.reduce_counts(eng.acc)
        if self.reducer.enabled and not self.use_graph:
            # graphs off on every rank (use_graph is configuration, identical across ranks): one bucket per decoder layer, launched from
            # the C callback as that layer's kernels are enqueued
            saved, self.bwd_pieces = self.bwd_pieces, 1
            try:
                self._part_bwd(0, per_layer_cb=self.reducer.layer_done)
            finally:
                self.bwd_pieces = saved
        else:
            # with graphs on, a rank may be in this eager step (first sight of an input signature, more signatures than graph slots, a
            # dropped graph) while another replays: both issue the SAME collectives -- one all-reduce per backward piece, same slices,
            # same order (_replay) -- so ranks never have to agree on eager vs replay.
            for i in range(self.bwd_pieces):
                self._part_bwd(i)
                hi, lo = self._piece_range(i)
                self.reducer.layers_done(lo, hi)
        if self.train_connectors:
            self.reducer.bucket_done(self.model.conn_g)      # one more bucket after the last backward piece, in every step path alike
        self.reducer.finish()
        self._part_opt()

    def _capture(self, audio, video, labels, prompt, micro=False):
        """Capture the step for this input signature.  Static input buffers are allocated here (the caller's tensors are copied into
        them before every replay -- or ARE them, see static_inputs()).  micro: the micro-step of a gradient-accumulation window instead
        (forward, backward pieces, accumulate; no optimizer part -- _close_window has its own graph)."""
        fwd, bwd = (self._part_micro_fwd, self._part_micro_bwd) if micro else (self._part_fwd, self._part_bwd)
        dev = self.model.llm_engine.lora_p.device
        st = {"inputs": [None if t is None else torch.empty(t.shape, dtype=t.dtype, device=dev) for t in (audio, video, labels, prompt)]}
        for dst, src in zip(st["inputs"], (audio, video, labels, prompt)):
            if dst is not None:
                dst.copy_(src)
        st["generation"] = Workspace.generation          # the graphs below hold raw pointers into the engines' workspaces as they are NOW
        pool = torch.cuda.graph_pool_handle()
        a, v, lab, pr = st["inputs"]
        torch.cuda.synchronize()
        if not self.reducer.enabled:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool):
                fwd(a, v, lab, pr)
                for i in range(self.bwd_pieces):
                    bwd(i)
                if not micro:
                    self._part_opt()
            st["all"] = g
        else:
            st["fwd"] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(st["fwd"], pool=pool):
                fwd(a, v, lab, pr)
            st["bwd"] = []
            for i in range(self.bwd_pieces):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, pool=pool):
                    bwd(i)
                st["bwd"].append(g)
            if not micro:
                st["opt"] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(st["opt"], pool=pool):
                    self._part_opt()
        st["modes"] = self.model.last_modality_modes          # the static mode buffer this signature's graph writes (None without modes)
        return st

    def _replay(self, st):
        if "all" in st:
            st["all"].replay()
            return
        eng = self.model.llm_engine
        st["fwd"].replay()
        self.reducer.reduce_counts(eng.acc)
        for i, g in enumerate(st["bwd"]):
            g.replay()
            hi, lo = self._piece_range(i)
            self.reducer.layers_done(lo, hi)
        if self.train_connectors:
            self.reducer.bucket_done(self.model.conn_g)
        self.reducer.finish()
        st["opt"].replay()

    def static_inputs(self, audio, video, labels, prompt):
        """The device buffers a captured step reads for inputs of this signature (None before it has been captured).  A feeder that
        writes its batches straight into them (H2D or a device-side producer) saves the per-step copy."""
        st = self._graphs.get(self._signature(audio, video, labels, prompt))
        return st["inputs"] if isinstance(st, dict) else None

    @staticmethod
    def _signature(*tensors):
        return tuple(None if t is None else (tuple(t.shape), t.dtype) for t in tensors)

    def _graph_state(self, audio, video, labels, prompt, micro=False):
        """The captured graphs of this input signature, or the reason this call runs eager ("warm", "stale", None): warm -> capture ->
        replay, at most 4 signatures."""
        key = self._signature(audio, video, labels, prompt)
        st = self._graphs.get(key)
        if isinstance(st, dict) and st["generation"] != Workspace.generation:
            # some workspace was reallocated since capture (a larger batch / more frames / generate() in between): every captured
            # graph may point into freed memory.  Drop them all; each signature is re-captured at its next-but-one visit.
            self._graphs = {k: "warm" for k in self._graphs}
            st = "stale"                             # this call runs eager and re-sizes nothing (workspaces only grow)
        if st is None and len(self._graphs) < 4:
            self._graphs[key] = st = "warm"          # first sight of a signature: eager (sizes every workspace); captured at the second
        elif st == "warm":
            self._graphs[key] = st = self._capture(audio, video, labels, prompt, micro=micro)
            if st["generation"] != Workspace.generation:         # cannot happen (Workspace.get refuses to grow under capture); belt and braces
                self._graphs[key] = st = "warm"
        return st

    def train_step(self, audio, video, labels, prompt, graph=None):
        """One optimizer step on this rank's batch; returns the (global) mean loss as a device scalar.
        graph=False forces the eager launch sequence for this call (bench.py's instrumented steps).
        With grad_accum_steps = N > 1 a call is a micro-step: forward, backward, accumulate, and it returns THIS rank's mean loss of the
        micro-batch; every N-th call (micro_step N-1) also closes the window -- one optimizer step on the concatenation of its N
        micro-batches over all ranks -- after which global_step is one higher and window_loss holds the window's global token-mean."""
        use_graph = self.use_graph if graph is None else (graph and self.use_graph)
        if isinstance(labels, list):
            labels = self.model._prep_labels(labels).cpu()
        if self.grad_accum_steps > 1:
            return self._micro_train_step(audio, video, labels, prompt, use_graph)
        self.global_step += 1
        st = self._graph_state(audio, video, labels, prompt) if use_graph else None
        if isinstance(st, dict):
            for dst, src in zip(st["inputs"], (audio, video, labels, prompt)):
                if dst is not None and src.data_ptr() != dst.data_ptr():
                    dst.copy_(src, non_blocking=True)
            self._replay(st)
            self.model.last_modality_modes = st["modes"]
        else:
            self._eager_step(audio, video, labels, prompt)
        return self._loss_buf.clone()

    @property
    def skipped_steps(self):
        return int(self.skipped.item())

    def _sync_step(self):
        """global_step := the optimizer steps actually taken (device-side count: skipped steps do not advance it).  One host sync; called
        where the host already waits for the device (log interval, checkpoint).  Mid-window (grad_accum_steps > 1) the device count already
        includes the step the open window will take (avllm_step_advance_micro advances it at micro-step 0): that one is not counted."""
        if self.grad_accum_steps > 1:
            words = self.state.view(torch.int32).cpu()
            taken = int(words[0]) - (1 if int(words[6]) > 0 else 0)                     # words[6]: reserved[0], the open window's micro-steps
        else:
            taken = int(self.state.view(torch.int32)[0].item())
        self._augment_skew += (self.global_step - taken) * self.grad_accum_steps         # the augmentation index stays where it is
        self.global_step = taken
        return self.global_step

    def _all_ranks_ok(self, ok):
        """Data-parallel runs: a batch is trained on only if EVERY rank could unpack its share -- a rank that skipped on its own would
        leave the others waiting in the step's all-reduces.  One 1-element MIN all-reduce per batch, only when distributed."""
        if not is_dist():
            return ok
        flag = torch.tensor([1.0 if ok else 0.0], device=self.model.llm_engine.lora_p.device)
        torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MIN)
        return bool(flag.item() > 0.5)

    def _train_epoch(self, epoch):
        self.model.train()
        total, n, t0 = 0.0, 0, time.time()
        pending, pending_modes, pending_noise, pending_video = [], [], [], []
        failures = unstable = worst = 0
        accum, windows = self.grad_accum_steps > 1, 0

        def examine(i):
            """Read the pending losses (one host sync), count them, apply the unstable-streak rule and log.  True: stop the epoch."""
            nonlocal total, n, unstable, worst
            vals = torch.stack(pending).float().cpu()
            pending.clear()
            self._sync_step()
            fin = torch.isfinite(vals)
            ok = vals[fin]
            total += float(ok.sum()); n += int(ok.numel())
            # trainer :444-452: a NaN loss skips the batch; more than 5 unstable batches in a row stop the epoch.  The losses stay on
            # the device between log intervals (no per-step host sync), so the streak is examined here, over the interval just read.
            for f in fin.tolist():
                unstable = 0 if f else unstable + 1
                worst = max(worst, unstable)
            if not bool(fin.all()):
                logging.warning(f"NaN loss detected in {int((~fin).sum())} {'window(s)' if accum else 'batch(es)'} up to batch {i}; {self.skipped_steps} optimizer step(s) skipped so far")
            if worst > 5:
                logging.error("Too many unstable batches. Stopping epoch.")
                return True
            what = f"window {windows} (batch {i + 1}/{len(self.train_dataloader)})" if accum else f"batch {i + 1}/{len(self.train_dataloader)}"
            where = f"window {windows}" if accum else f"batch {i + 1}"          # the shares below cover every micro-batch since the last look
            nll = f"nll {float(self.last_nll):.4f} " if self.last_nll is not None else ""      # the last (micro-)batch's, on this rank
            logging.info(f"epoch {epoch} {what} loss {float(vals[-1]):.4f} {nll}"
                         f"avg {total / max(1, n):.4f} lr {self.lr_at(self.global_step):.3e} {(time.time() - t0) / (i + 1):.3f}s/it")
            if pending_modes:
                share = self.mode_shares(torch.cat(pending_modes).cpu())
                pending_modes.clear()
                logging.info(f"epoch {epoch} {where}: clips with both streams {share[0]:.3f}, audio only {share[1]:.3f}, video only {share[2]:.3f}")
            if pending_noise:
                share, snr = self.noise_shares(torch.cat(pending_noise).cpu())
                pending_noise.clear()
                logging.info(f"epoch {epoch} {where}: clips with noise mixed in {share:.3f}, their mean SNR {snr:.2f} dB")
            if pending_video:
                flipped, masked = self.video_shares(torch.cat([v[0] for v in pending_video]).cpu(),
                                                    [n for v in pending_video for n in (v[1].tolist() if torch.is_tensor(v[1]) else v[1])])
                pending_video.clear()
                logging.info(f"epoch {epoch} {where}: clips flipped {flipped:.3f}, mean share of frames masked {masked:.3f}")
            return False

        for i, batch in enumerate(self.train_dataloader):
            # the reference logs and skips a batch on ANY exception (:492-507).  Host-side preparation (everything before the first
            # collective) is where data errors surface; under DDP the skip is agreed between ranks first.
            unpacked, err = None, None
            self.last_augment_info = self.last_video_info = None
            try:
                unpacked = self._unpack(batch)
            except Exception as e:
                err = e
            if not self._all_ranks_ok(err is None):
                logging.error(f"Error in batch {i}: {err if err is not None else 'another rank failed to prepare its batch'}")
                failures += 1
                if failures > 5:
                    raise RuntimeError("more than 5 consecutive batches failed") from err
                continue
            try:
                loss = self.train_step(*unpacked)
            except Exception as e:                               # the reference logs and skips on ANY exception (:492-507)
                if is_dist():
                    raise                                        # mid-step: the other ranks are already inside the collectives
                logging.error(f"Error in batch {i}: {e}")
                if accum:
                    logging.error(f"the open window is abandoned with {self._abandon_window()} micro-batch(es) in it")
                failures += 1
                if failures > 5:
                    raise RuntimeError("more than 5 consecutive batches failed") from e
                continue
            failures = 0
            if accum:
                # the loss that is logged and examined is the WINDOW's (the 5-in-a-row rule counts windows); a partial last window of the
                # epoch is closed here, so no gradient leaks into the next epoch and no micro-batch is dropped
                if i + 1 == len(self.train_dataloader):
                    self.flush()
                if self.micro_step == 0:
                    windows += 1
                    pending.append(self.window_loss.clone())
            else:
                pending.append(loss)
            if self.model.last_modality_modes is not None:       # stays on the device until the log interval, like the loss
                pending_modes.append(self.model.last_modality_modes.clone())
            if self.last_augment_info is not None:               # a tensor of its own per batch: kept, not copied
                pending_noise.append(self.last_augment_info)
            if self.last_video_info is not None:
                pending_video.append(self.last_video_info)
            if accum:                                            # log_interval counts optimizer steps: look when a window has just closed
                due = bool(pending) and ((self.micro_step == 0 and windows % self.log_interval == 0) or i + 1 == len(self.train_dataloader))
            else:
                due = (i + 1) % self.log_interval == 0 or i + 1 == len(self.train_dataloader)
            if due and examine(i):
                break
        if accum and (self.micro_step > 0 or pending):
            # the epoch ended on a batch that was skipped: the open window still becomes a step (every rank takes this path alike: skips are
            # agreed between ranks), and it is examined, counted and logged like every other window
            if self.micro_step > 0:
                self.flush()
                windows += 1
                pending.append(self.window_loss.clone())
            examine(i)
        return total / max(1, n)

    @staticmethod
    def noise_shares(info):
        """(the share of clips with noise mixed in, their mean requested SNR in dB -- nan when there is none) of AudioAugment.last_info rows."""
        info = info.contiguous()
        on = info[:, 0] != 0
        snr = info.view(torch.float32)[:, 3][on]
        return float(on.float().mean()) if info.shape[0] else 0.0, float(snr.mean()) if snr.numel() else float("nan")

    @staticmethod
    def video_shares(info, frames):
        """(the share of clips flipped, the mean over clips of masked frames / the clip's frames) of VideoAugment.last_info rows and the clips'
        frame counts; a clip without frames counts as unmasked."""
        if not info.shape[0]:
            return 0.0, 0.0
        share = [m / n if n > 0 else 0.0 for m, n in zip(info[:, 3].tolist(), frames)]
        return float((info[:, 2] != 0).float().mean()), sum(share) / len(share)

    @staticmethod
    def mode_shares(modes):
        """The share of clips in mode 0 (both), 1 (audio only) and 2 (video only) of an int32 tensor of modes; any other value counts as 0."""
        n = max(1, modes.numel())
        one, two = int((modes == 1).sum()), int((modes == 2).sum())
        return [(modes.numel() - one - two) / n, one / n, two / n]

    @torch.no_grad()
    def _validate(self):
        if self.val_dataloader is None:
            return None
        self.model.eval()
        tot, cnt = 0.0, 0
        for batch in self.val_dataloader:
            audio, video, labels, prompt = self._unpack(batch)
            out = self.model(audio=audio, video=video, prompt=prompt, labels=labels, return_loss=True)
            bs = labels.shape[0]
            v = float(out["loss"])
            if math.isfinite(v):
                tot += v * bs; cnt += bs
        self.model.train()
        return tot / max(1, cnt)

    def _lora_keys(self):
        """peft-named LoRA keys in the order torch's optimizer indexes them (state-dict order: per layer the adapted modules out of q,k,v,o,
        gate,up,down; A then B) == the order of the flat LoRA buffer."""
        eng = self.model.llm_engine
        from .arch import lora_state_key
        return [lora_state_key(i, nm, ab) for i in range(eng.cfg.layers) for nm in eng.targets for ab in ("lora_A", "lora_B")]

    def _save_checkpoint(self, epoch, name):
        """Same top-level keys as trainer:752-760.  model_state_dict holds the tensors this build owns (connectors + LoRA under peft's key
        names: decode.py:236-260 extracts the connectors by substring); the frozen encoders / LLM the reference also dumps into every
        checkpoint (13.5 GB for a 7B LLM) are not repeated -- they are the checkpoints the model was built from.  optimizer_state_dict /
        scheduler_state_dict follow torch.optim.AdamW / CosineAnnealingLR's own layout for the LoRA parameters, in optimizer index order."""
        if self.grad_accum_steps > 1 and self.micro_step > 0:
            # checkpoints are written at window boundaries only (the file has no place for half a window's gradient sums): a save asked for
            # mid-window, on every rank alike, waits for the closing micro-step or flush()
            self._deferred_save = (epoch, name)
            return
        if is_dist() and torch.distributed.get_rank() != 0:
            return
        os.makedirs(self.output_dir, exist_ok=True)
        self._sync_step()
        path = os.path.join(self.output_dir, name)
        eng = self.model.llm_engine
        state, n = {}, 0
        no_decay = []
        if self.train_connectors:
            # connectors first, then LoRA: named_parameters() order, as a torch optimizer over the reference's parameter list numbers them
            for cm, cv, (_, _, shape) in zip(self.model.connector_grad_views(self.cm), self.model.connector_grad_views(self.cv), self.model.conn_slices):
                state[n] = {"step": torch.tensor(float(self.global_step)), "exp_avg": cm.detach().cpu().clone(), "exp_avg_sq": cv.detach().cpu().clone()}
                if len(shape) == 1:
                    no_decay.append(n)
                n += 1
        mv, vv = eng.lora_views(self.m), eng.lora_views(self.v)
        for key in self._lora_keys():
            _, _, _, _, _, li, _, mod, ab, _, _ = key.split(".")
            short = f"layers.{li}.{mod}.{ab}"
            state[n] = {"step": torch.tensor(float(self.global_step)), "exp_avg": mv[short].detach().cpu().clone(), "exp_avg_sq": vv[short].detach().cpu().clone()}
            n += 1
        group = {"lr": self.lr_at(self.global_step), "betas": (0.9, 0.95), "eps": 1e-8, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None, "initial_lr": self.learning_rate,
                 "params": [i for i in range(n) if i not in no_decay]}
        groups = [group] + ([dict(group, weight_decay=0.0, params=no_decay)] if no_decay else [])      # biases: weight_decay 0 (:183-197)
        torch.save({"epoch": epoch, "model_state_dict": self.model.state_dict(),
                    "optimizer_state_dict": {"state": state, "param_groups": groups},
                    "scheduler_state_dict": {"T_max": self.total_steps, "eta_min": 0.0, "base_lrs": [self.learning_rate], "last_epoch": self.global_step,
                                             "_step_count": self.global_step + 1, "_last_lr": [self.lr_at(self.global_step)]},
                    "train_losses": self.train_losses, "val_losses": self.val_losses, "best_val_loss": self.best_val_loss}, path)
        json.dump({"epoch": epoch, "global_step": self.global_step, "best_val_loss": self.best_val_loss, "grad_accum_steps": self.grad_accum_steps,
                   "augment_index": self._augment_index(), "skipped_steps": self.skipped_steps, "lora_target_modules": list(self.model.lora_target_modules) if self.model.use_lora else None,
                   "label_smoothing": self.label_smoothing, "z_loss": self.z_loss},
                  open(path.replace(".pt", "_meta.json"), "w"))

    @staticmethod
    def checkpoint_lora_targets(path):
        """The lora_target_modules a checkpoint of _save_checkpoint() was trained with, from the `_meta.json` beside it; None when the file or
        the entry is absent (a checkpoint of the reference trainer, or of a build before the keyword: the default four).  A resume builds
        its model with this (scripts/clip_whisper/train.py --resume_from)."""
        meta = str(path).replace(".pt", "_meta.json")
        if not os.path.exists(meta):
            return None
        t = json.load(open(meta)).get("lora_target_modules")
        return None if t is None else list(t)

    @staticmethod
    def _meta_count(path, key):
        meta = str(path).replace(".pt", "_meta.json")
        if not os.path.exists(meta):
            return None
        n = json.load(open(meta)).get(key)
        return None if n is None else int(n)

    @staticmethod
    def checkpoint_loss_options(path):
        """(label_smoothing, z_loss) a checkpoint of _save_checkpoint() was trained with, from the `_meta.json` beside it; None when the file or
        the entries are absent (a checkpoint of the reference trainer, or of a build before the options)."""
        meta = str(path).replace(".pt", "_meta.json")
        if not os.path.exists(meta):
            return None
        d = json.load(open(meta))
        if "label_smoothing" not in d and "z_loss" not in d:
            return None
        return float(d.get("label_smoothing") or 0.0), float(d.get("z_loss") or 0.0)

    @classmethod
    def checkpoint_augment_index(cls, path):
        """The augmentation index (_augment_index) a checkpoint of _save_checkpoint() was written at, from the `_meta.json` beside it; None when
        the file or the entry is absent (a checkpoint of the reference trainer, or of a build before the entry)."""
        return cls._meta_count(path, "augment_index")

    @classmethod
    def checkpoint_skipped_steps(cls, path):
        """The optimizer steps the run had skipped on a non-finite loss or gradient when the checkpoint was written (`_meta.json`); None when
        the file or the entry is absent.  The count is part of every step's dropout seed (avllm_step_state)."""
        return cls._meta_count(path, "skipped_steps")

    def load_checkpoint(self, path):
        """trainer:796-854.  Reads a checkpoint of this build AND one written by the reference trainer: connectors + LoRA from
        model_state_dict, Adam moments from torch's optimizer state (the only parameters with state are the ones that ever received a
        gradient -- the LoRA tensors, SURVEY.md fact 4 -- in state-dict order), the step count from the scheduler's last_epoch."""
        saved = self.checkpoint_lora_targets(path)
        if saved is not None and self.model.use_lora and tuple(saved) != tuple(self.model.lora_target_modules):
            raise ValueError(f"load_checkpoint(): {path} was trained with lora_target_modules = {', '.join(saved)}, this model has "
                             f"{', '.join(self.model.lora_target_modules)}: build the model with checkpoint_lora_targets(path)")
        opts = self.checkpoint_loss_options(path)
        if opts is not None and opts != (self.label_smoothing, self.z_loss):
            # the objective is not part of the state: the run goes on under the trainer's values, and its losses no longer compare
            logging.warning(f"load_checkpoint(): {path} was trained with label_smoothing={opts[0]}, z_loss={opts[1]}; this trainer goes on with "
                            f"label_smoothing={self.label_smoothing}, z_loss={self.z_loss}")
        ck = torch.load(path, map_location="cpu", weights_only=True)
        self.model.load_state_dict(ck["model_state_dict"])
        eng = self.model.llm_engine
        o = ck.get("optimizer_state_dict") or {}
        step = None
        if "m" in o:                                             # round-1 layout of this build
            self.m.copy_(o["m"]); self.v.copy_(o["v"]); step = int(o.get("step", 0))
        elif "state" in o:
            ids = sorted(int(k) for k, st in o["state"].items() if isinstance(st, dict) and "exp_avg" in st)
            keys = self._lora_keys()
            if self.train_connectors and len(ids) == len(keys) + 4:      # connectors first (named_parameters() order), then LoRA
                cms, cvs = self.model.connector_grad_views(self.cm), self.model.connector_grad_views(self.cv)
                for idx, cm, cv in zip(ids[:4], cms, cvs):
                    st = o["state"][idx] if idx in o["state"] else o["state"][str(idx)]
                    if tuple(st["exp_avg"].shape) != tuple(cm.shape):
                        raise ValueError(f"optimizer state {idx} has shape {tuple(st['exp_avg'].shape)}, the connector tensor is {tuple(cm.shape)}")
                    cm.copy_(st["exp_avg"]); cv.copy_(st["exp_avg_sq"])
                ids = ids[4:]
            if len(ids) != len(keys):
                raise ValueError(f"optimizer state has {len(ids)} tensors with moments, the model has {len(keys)} LoRA tensors")
            mv, vv = eng.lora_views(self.m), eng.lora_views(self.v)
            for idx, key in zip(ids, keys):
                st = o["state"][idx] if idx in o["state"] else o["state"][str(idx)]
                _, _, _, _, _, li, _, mod, ab, _, _ = key.split(".")
                short = f"layers.{li}.{mod}.{ab}"
                if tuple(st["exp_avg"].shape) != tuple(mv[short].shape):
                    raise ValueError(f"optimizer state {idx} has shape {tuple(st['exp_avg'].shape)}, {key} is {tuple(mv[short].shape)}")
                mv[short].copy_(st["exp_avg"]); vv[short].copy_(st["exp_avg_sq"])
                step = int(float(st["step"]))
        sched = ck.get("scheduler_state_dict") or {}
        if "last_epoch" in sched:
            step = int(sched["last_epoch"])
        elif "step" in sched:
            step = int(sched["step"])
        if step is not None:
            self.global_step = step
            self.state.view(torch.int32)[0] = step                 # the device-side step count drives lr / bias corrections / seeds
        if self.grad_accum_steps > 1:                            # a checkpoint is a window boundary: training resumes at micro-step 0
            self.micro_step, self._deferred_save = 0, None
            self.state.view(torch.int32)[6] = 0
        # the augmentation index the run had reached (_augment_index); a checkpoint without the entry: global_step * grad_accum_steps
        # the steps skipped so far: the seed of a step's LoRA dropout masks and modality modes is a function of step + skipped, so a resumed
        # run draws what the uninterrupted one draws only with the count restored (without the entry: 0, as before)
        skipped = self.checkpoint_skipped_steps(path)
        if skipped is not None:
            self.skipped.fill_(float(skipped))
            self.state.view(torch.float32)[5] = float(skipped)
        index = self.checkpoint_augment_index(path)
        self._augment_skew = 0 if index is None else index - self.global_step * self.grad_accum_steps
        self.train_losses, self.val_losses = list(ck.get("train_losses", [])), list(ck.get("val_losses", []))
        self.best_val_loss = ck.get("best_val_loss", float("inf"))
        return ck.get("epoch", 0)

    def train(self):
        os.makedirs(self.output_dir, exist_ok=True)
        t0 = time.time()
        log_csv = os.path.join(self.output_dir, "loss_log.csv")
        with open(log_csv, "w", newline="") as f:
            csv.writer(f).writerow(["epoch", "train_loss", "val_loss", "time_hours", "remaining_hours"])
        for epoch in range(self.max_epochs):
            tl = self._train_epoch(epoch)
            vl = self._validate()
            self.train_losses.append(tl)
            if vl is not None:
                self.val_losses.append(vl)
                if vl < self.best_val_loss:
                    self.best_val_loss = vl
                    self._save_checkpoint(epoch, "model_best.pt")
            if (epoch + 1) % self.save_every == 0:
                self._save_checkpoint(epoch, f"checkpoint_epoch_{epoch + 1}.pt")
            el = (time.time() - t0) / 3600
            with open(log_csv, "a", newline="") as f:
                csv.writer(f).writerow([epoch + 1, tl, vl, el, el / (epoch + 1) * (self.max_epochs - epoch - 1)])
        self._save_checkpoint(self.max_epochs - 1, "model_final.pt")
        return {"train_losses": self.train_losses, "val_losses": self.val_losses, "best_val_loss": self.best_val_loss,
                "training_hours": (time.time() - t0) / 3600}
