"""Device-side feature extraction: raw 16 kHz samples and raw RGB uint8 frames in, the model's inputs out.

Mirrors what `AVSRDataset.__getitem__` does per sample on CPU workers (src/clip_whisper/data/simple_dataset.py:156-186,
:191-264) and what `collate_fn` does per batch (:317-460: stack audio, zero-pad video to the longest clip), on the GPU and per
batch: `WhisperLogMel` = `whisper_processor(audio, sampling_rate=16000).input_features` + `F.layer_norm(f, f.shape)`;
`ClipFrames` = `clip_processor(images=frame)["pixel_values"]`.  Decoding files (soundfile / cv2) stays with the caller."""
import ctypes as C
import os

import numpy as np
import torch

from . import lib as L

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
N_SAMPLES, N_MELS, N_FRAMES = 480000, 80, 3000


class WhisperLogMel:
    def __init__(self, device="cuda:0", normalize=True, n_mels=N_MELS):
        """n_mels: 80 (Whisper tiny..large-v2) or 128 (large-v3's feature extractor, feature_size=128)."""
        self.device, self.normalize, self.n_mels = torch.device(device), normalize, int(n_mels)
        lib = L.load()
        self.table = torch.empty(lib.avllm_logmel_table_bytes(), dtype=torch.uint8, device=self.device)
        L.check(lib.avllm_logmel_table_init(L.ptr(self.table), self.n_mels))
        self._ws = None

    def pad_batch(self, waves, return_lengths=False):
        """list of 1-D float arrays/tensors (mono, 16 kHz, any length) -> one zero-padded [B, n] float32 device tensor; with return_lengths
        also the clips' sample counts (after the 30 s cut) as an int32 [B] device tensor."""
        waves = [torch.as_tensor(np.asarray(w, dtype=np.float32) if not torch.is_tensor(w) else w, dtype=torch.float32).reshape(-1)[:N_SAMPLES]
                 for w in waves]
        n = max(1, max(int(w.numel()) for w in waves))
        out = torch.zeros(len(waves), n, dtype=torch.float32, device=self.device)
        for i, w in enumerate(waves):
            out[i, : w.numel()] = w.to(self.device, non_blocking=True)
        if return_lengths:
            return out, torch.tensor([int(w.numel()) for w in waves], dtype=torch.int32, device=self.device)
        return out

    def __call__(self, wave, out=None):
        """wave: [B, n] float32 (rows zero-padded) or a list of 1-D waveforms -> [B, n_mels, 3000] float32 on the device
        (written into `out` when given: a feeder filling a captured step's input buffer)."""
        if isinstance(wave, (list, tuple)):
            wave = self.pad_batch(wave)
        if wave.dim() == 1:
            wave = wave[None]
        if wave.dim() != 2:
            raise ValueError(f"waveform batch should have shape [batch_size, samples], but got {tuple(wave.shape)}")
        wave = wave.to(self.device, torch.float32).contiguous()
        B, n = wave.shape
        lib = L.load()
        need = lib.avllm_logmel_workspace_bytes(B, self.n_mels)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if out is None:
            out = torch.empty(B, self.n_mels, N_FRAMES, dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (B, self.n_mels, N_FRAMES) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != wave.device:
            raise ValueError(f"out should be a contiguous float32 [{B}, {self.n_mels}, {N_FRAMES}] tensor on {wave.device}, but got {out.dtype} {tuple(out.shape)}")
        L.check(lib.avllm_logmel(L.ptr(self.table), L.ptr(wave), B, n, wave.stride(0), int(self.normalize), self.n_mels, L.ptr(out),
                                 L.ptr(self._ws), self._ws.numel(), L.stream_ptr()))
        return out


class ClipFrames:
    def __init__(self, device="cuda:0", image=224, mean=CLIP_MEAN, std=CLIP_STD, dtype=torch.float32):
        self.device, self.image, self.dtype = torch.device(device), image, dtype
        self.mean = (C.c_float * 3)(*mean)
        self.std = (C.c_float * 3)(*std)
        self._plans, self._ws = {}, None
        self._aug_plans = {}                          # (H, W, resize) -> plan of avllm_clip_preproc_aug (VideoAugment.frames)

    def _aug_plan(self, H, W, resize):
        key = (H, W, resize)
        if key not in self._aug_plans:
            lib = L.load()
            buf = torch.empty(lib.avllm_clip_preproc_aug_plan_bytes(H, W, resize, self.image), dtype=torch.uint8, device=self.device)
            L.check(lib.avllm_clip_preproc_aug_plan_init(L.ptr(buf), H, W, resize, self.image, self.mean, self.std))
            self._aug_plans[key] = buf
        return self._aug_plans[key]

    def _plan(self, H, W):
        key = (H, W)
        if key not in self._plans:
            lib = L.load()
            buf = torch.empty(lib.avllm_clip_preproc_plan_bytes(H, W, self.image), dtype=torch.uint8, device=self.device)
            L.check(lib.avllm_clip_preproc_plan_init(L.ptr(buf), H, W, self.image, self.mean, self.std))
            self._plans[key] = buf
        return self._plans[key]

    def __call__(self, frames, out=None):
        """frames: uint8 [N, H, W, 3] RGB (any H, W) -> pixel_values [N, 3, image, image] (written into `out` when given)."""
        frames = torch.as_tensor(frames)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f"frames should be uint8 [frames, height, width, 3], but got {frames.dtype} {tuple(frames.shape)}")
        frames = frames.to(self.device).contiguous()
        N, H, W, _ = frames.shape
        lib = L.load()
        plan = self._plan(H, W)
        need = lib.avllm_clip_preproc_workspace_bytes(N, H, W, self.image)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        if out is None:
            out = torch.empty(N, 3, self.image, self.image, dtype=self.dtype, device=self.device)
        elif out.numel() != N * 3 * self.image * self.image or out.dtype != self.dtype or not out.is_contiguous() or out.device != frames.device:
            raise ValueError(f"out should be a contiguous {self.dtype} tensor of {N} x 3 x {self.image} x {self.image} elements on {frames.device}, "
                             f"but got {out.dtype} {tuple(out.shape)}")
        L.check(lib.avllm_clip_preproc(L.ptr(plan), L.ptr(frames), N, H, W, self.image, L.ptr(out), L.dt_of(out), L.ptr(self._ws),
                                       self._ws.numel(), L.stream_ptr()))
        return out


class NoiseBank:
    """The noise recordings avllm_wave_add_noise draws from, as one zero-padded float32 image [Nn, W] and their lengths (int32 [Nn]) on the
    device.  `sources`: a .wav / .npy file, a directory of them (sorted by name), or a list of arrays (or of paths).  Files are read with
    avllm.data.read_audio and brought to mono float32 the way AVSRDataset brings a clip (mean over channels, int16-range values / 32768); a
    file at any other rate than 16 kHz is a ValueError that names it: there is no resampler."""

    def __init__(self, sources, device="cuda:0", sampling_rate=16000):
        self.device = torch.device(device)
        self.path = sources if isinstance(sources, (str, os.PathLike)) else None
        if isinstance(sources, (str, os.PathLike)):
            p = os.fspath(sources)
            if os.path.isdir(p):
                sources = [os.path.join(p, f) for f in sorted(os.listdir(p)) if f.lower().endswith((".wav", ".npy"))]
                if not sources:
                    raise ValueError(f"{p}: no .wav / .npy noise recordings in this directory")
            else:
                sources = [p]
        rows, self.names = [], []
        for i, s in enumerate(sources):
            if isinstance(s, (str, os.PathLike)):
                from .data import read_audio
                x, sr = read_audio(os.fspath(s))
                if int(sr) != sampling_rate:
                    raise ValueError(f"{s}: noise at {sr} Hz, the clips are {sampling_rate} Hz (resample the file; nothing here does)")
                name = os.fspath(s)
            else:
                x, name = (s.detach().cpu().numpy() if torch.is_tensor(s) else s), f"array {i}"
            x = np.asarray(x)
            if x.ndim > 1:
                x = x.mean(axis=1)
            x = x.astype(np.float32) / 32768.0 if np.abs(x).max(initial=0.0) > 1.0 else x.astype(np.float32)
            if x.size < 1:
                raise ValueError(f"{name}: an empty noise recording")
            rows.append(np.ascontiguousarray(x.reshape(-1)))
            self.names.append(name)
        if not rows:
            raise ValueError("NoiseBank: no noise recordings given")
        width = (max(r.size for r in rows) + 3) // 4 * 4
        image = np.zeros((len(rows), width), np.float32)
        for i, r in enumerate(rows):
            image[i, : r.size] = r
        self.noise = torch.from_numpy(image).to(self.device)
        self.lengths = torch.tensor([r.size for r in rows], dtype=torch.int32, device=self.device)

    def __len__(self):
        return self.noise.shape[0]


class AudioAugment:
    """The two acoustic augmentations (include/avllm.h, avllm_wave_add_noise and avllm_spec_augment; csrc/augment.hip).
    noise: a NoiseBank | None; snr_db: (lo, hi), drawn per clip, or one value; noise_prob: the share of clips that get noise.
    time_masks x [0, min(time_width, time_ratio * frames)] frames and freq_masks x [0, freq_width] mel bins are set to `fill`: 0.0 is the clip's
    mean after the whole-tensor layer norm, and what transformers' Whisper `_mask_input_features` writes."""

    def __init__(self, noise=None, snr_db=(0.0, 20.0), noise_prob=1.0, time_masks=0, time_width=0, time_ratio=1.0, freq_masks=0, freq_width=0,
                 fill=0.0):
        lo, hi = (snr_db, snr_db) if isinstance(snr_db, (int, float)) else snr_db
        self.noise, self.snr_lo, self.snr_hi, self.noise_prob = noise, float(lo), float(hi), float(noise_prob)
        self.time_masks, self.time_width, self.time_ratio = int(time_masks), int(time_width), float(time_ratio)
        self.freq_masks, self.freq_width, self.fill = int(freq_masks), int(freq_width), float(fill)
        if self.snr_lo > self.snr_hi:
            raise ValueError(f"AudioAugment: snr_db = ({self.snr_lo}, {self.snr_hi}): the lower end is above the upper one")
        if not 0.0 <= self.noise_prob <= 1.0:
            raise ValueError(f"AudioAugment: noise_prob = {self.noise_prob} must lie in [0, 1]")
        if min(self.time_masks, self.freq_masks, self.time_width, self.freq_width) < 0 or self.time_masks + self.freq_masks > 32:
            raise ValueError(f"AudioAugment: time_masks = {self.time_masks}, freq_masks = {self.freq_masks} (at most 32 together), time_width = "
                             f"{self.time_width}, freq_width = {self.freq_width}: none may be negative")
        if not 0.0 <= self.time_ratio <= 1.0:
            raise ValueError(f"AudioAugment: time_ratio = {self.time_ratio} must lie in [0, 1]")
        self.last_info = self.last_spans = None      # device tensors of the last .wave() / .features() call: int32 [B, 5] / int32 [B, masks, 2]
        self._ws = None

    @property
    def mixes(self):
        return self.noise is not None

    @property
    def masks(self):
        return self.time_masks + self.freq_masks > 0

    @staticmethod
    def _seed_ptr(seed_dev):
        if isinstance(seed_dev, torch.Tensor):
            if seed_dev.numel() != 1 or seed_dev.element_size() != 4:
                raise ValueError(f"AudioAugment: seed_dev must hold one 32-bit word, got {tuple(seed_dev.shape)} {seed_dev.dtype}")
            return L.ptr(seed_dev)
        return seed_dev

    def wave(self, batch, lengths=None, seed=0, seed_dev=None, snr_db=None, out=None):
        """batch f32 [B, n] on the device (any row stride), lengths int32 [B] on the device | None (= n) -> the batch with noise mixed in, in
        `out` (default a new tensor; `out=batch` mixes in place).  snr_db: a float32 [B] device tensor overrides the drawn values.  Without a
        noise bank the batch is returned as it is.  last_info: int32 [B, 5] = applied, row, offset and the bits of snr_db and gain."""
        if self.noise is None:
            return batch
        if batch.dim() != 2 or batch.dtype != torch.float32 or batch.stride(1) != 1 or not batch.is_cuda:
            raise ValueError(f"AudioAugment.wave: batch should be a float32 [batch_size, samples] device tensor with unit column stride, got {batch.dtype} {tuple(batch.shape)}")
        B, n = batch.shape
        if out is None:
            out = torch.empty(B, n, dtype=torch.float32, device=batch.device)
        elif tuple(out.shape) != (B, n) or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != batch.device:
            raise ValueError(f"AudioAugment.wave: out should be a float32 [{B}, {n}] tensor on {batch.device}, got {out.dtype} {tuple(out.shape)}")
        for nm, t, dt in (("lengths", lengths, torch.int32), ("snr_db", snr_db, torch.float32)):
            if t is not None and (t.dtype != dt or tuple(t.shape) != (B,) or not t.is_contiguous() or t.device != batch.device):
                raise ValueError(f"AudioAugment.wave: {nm} should be a contiguous {dt} [{B}] tensor on {batch.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        lib = L.load()
        need = lib.avllm_wave_add_noise_workspace_bytes(B, n)
        if self._ws is None or self._ws.numel() < need or self._ws.device != batch.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=batch.device)
        info = torch.empty(B, 5, dtype=torch.int32, device=batch.device)
        nb = self.noise
        L.check(lib.avllm_wave_add_noise(L.ptr(batch), batch.stride(0), L.ptr(lengths), B, n, L.ptr(nb.noise), nb.noise.stride(0), L.ptr(nb.lengths),
                                         len(nb), L.ptr(snr_db), self.snr_lo, self.snr_hi, self.noise_prob, int(seed) & 0xFFFFFFFF,
                                         self._seed_ptr(seed_dev), L.ptr(out), out.stride(0), L.ptr(info), L.ptr(self._ws), self._ws.numel(),
                                         L.stream_ptr()))
        self.last_info = info
        return out

    def features(self, feat, valid=None, seed=0, seed_dev=None):
        """SpecAugment IN PLACE on feat f32 [B, M, T] (contiguous, on the device); valid int32 [B] on the device | None (= T): the frames each
        clip really has.  Returns feat.  Without masks nothing is launched.  last_spans: int32 [B, time_masks + freq_masks, 2] = (start, width)."""
        if not self.masks:
            return feat
        if feat.dim() != 3 or feat.dtype != torch.float32 or not feat.is_contiguous() or not feat.is_cuda:
            raise ValueError(f"AudioAugment.features: feat should be a contiguous float32 [batch_size, mels, frames] device tensor, got {feat.dtype} {tuple(feat.shape)}")
        B, M, T = feat.shape
        if valid is not None and (valid.dtype != torch.int32 or tuple(valid.shape) != (B,) or not valid.is_contiguous() or valid.device != feat.device):
            raise ValueError(f"AudioAugment.features: valid should be a contiguous int32 [{B}] tensor on {feat.device}, got {valid.dtype} {tuple(valid.shape)} on {valid.device}")
        spans = torch.empty(B, self.time_masks + self.freq_masks, 2, dtype=torch.int32, device=feat.device)
        L.check(L.load().avllm_spec_augment(L.ptr(feat), B, M, T, L.ptr(valid), self.time_masks, self.time_width, self.time_ratio, self.freq_masks,
                                            self.freq_width, self.fill, int(seed) & 0xFFFFFFFF, self._seed_ptr(seed_dev), L.ptr(spans), L.stream_ptr()))
        self.last_spans = spans
        return feat

    @staticmethod
    def info_fields(info):
        """last_info (int32 [B, 5], on any device) -> dict of host lists: applied, row, offset (int) and snr_db, gain (float)."""
        info = info.cpu().contiguous()
        f = info.view(torch.float32)
        return {"applied": info[:, 0].tolist(), "row": info[:, 1].tolist(), "offset": info[:, 2].tolist(), "snr_db": f[:, 3].tolist(),
                "gain": f[:, 4].tolist()}


class VideoAugment:
    """The visual augmentations (include/avllm.h, "visual augmentation"; csrc/video_augment.hip), one draw per clip: the frames are resized so
    that the shorter edge is `resize` (None: the image size, i.e. no room to crop), a window of the image size is cut at a drawn corner
    (random_crop=False: the centre), the clip is mirrored with probability flip_prob, and time_masks spans of
    [0, min(time_width, time_ratio * frames)] frames are set to `fill` (0.0: the mean pixel after CLIP's normalisation, roughly)."""

    def __init__(self, resize=None, random_crop=True, flip_prob=0.5, time_masks=0, time_width=0, time_ratio=1.0, fill=0.0):
        self.resize = None if resize is None else int(resize)
        self.random_crop, self.flip_prob = bool(random_crop), float(flip_prob)
        self.time_masks, self.time_width, self.time_ratio, self.fill = int(time_masks), int(time_width), float(time_ratio), float(fill)
        if self.resize is not None and self.resize < 1:
            raise ValueError(f"VideoAugment: resize = {self.resize} must be at least 1 (None: the image size)")
        if not 0.0 <= self.flip_prob <= 1.0:
            raise ValueError(f"VideoAugment: flip_prob = {self.flip_prob} must lie in [0, 1]")
        if not 0 <= self.time_masks <= 16:
            raise ValueError(f"VideoAugment: time_masks = {self.time_masks} must lie in [0, 16]")
        if self.time_width < 0:
            raise ValueError(f"VideoAugment: time_width = {self.time_width} may not be negative")
        if not 0.0 <= self.time_ratio <= 1.0:
            raise ValueError(f"VideoAugment: time_ratio = {self.time_ratio} must lie in [0, 1]")
        # device tensors of the last call: int32 [clips, 4] = left, top, flip, masked / int32 [clips, time_masks, 2] = (start, width); and the
        # clips' frame counts as a host list (what `masked` is a share of)
        self.last_info = self.last_spans = self.last_frames = None
        self._ws = None

    _seed_ptr = staticmethod(AudioAugment._seed_ptr)

    def frames(self, clip_frames, frames, clip, seed, seed_dev=None, out=None, info=None, spans=None):
        """One clip through the fused path: frames uint8 [N, H, W, 3] -> pixel_values [N, 3, image, image] of clip_frames' image size and dtype
        (written into `out` when given).  clip: the clip's index in its batch.  info int32 [4] / spans int32 [time_masks, 2]: device rows to
        write the draw into (a batch's collector); without them last_info / last_spans are this clip's own [1, 4] / [1, time_masks, 2]."""
        frames = torch.as_tensor(frames)
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3:
            raise ValueError(f"frames should be uint8 [frames, height, width, 3], but got {frames.dtype} {tuple(frames.shape)}")
        cf, image = clip_frames, clip_frames.image
        resize = image if self.resize is None else self.resize
        if resize < image:
            raise ValueError(f"VideoAugment: resize = {resize} is below the image size {image}: the crop window must fit the resized frame")
        if int(clip) < 0:
            raise ValueError(f"VideoAugment.frames: clip = {clip} may not be negative")
        frames = frames.to(cf.device).contiguous()
        N, H, W, _ = frames.shape
        lib = L.load()
        plan = cf._aug_plan(H, W, resize)
        need = lib.avllm_clip_preproc_aug_workspace_bytes(N, H, W, resize, image)
        if self._ws is None or self._ws.numel() < need or self._ws.device != frames.device:
            self._ws = torch.empty(need, dtype=torch.uint8, device=frames.device)
        if out is None:
            out = torch.empty(N, 3, image, image, dtype=cf.dtype, device=frames.device)
        elif out.numel() != N * 3 * image * image or out.dtype != cf.dtype or not out.is_contiguous() or out.device != frames.device:
            raise ValueError(f"out should be a contiguous {cf.dtype} tensor of {N} x 3 x {image} x {image} elements on {frames.device}, "
                             f"but got {out.dtype} {tuple(out.shape)}")
        own = info is None
        if not own and self.time_masks and spans is None:
            raise ValueError(f"VideoAugment.frames: info is given but spans is not, with time_masks = {self.time_masks}: both rows or neither")
        if own:
            info = torch.empty(1, 4, dtype=torch.int32, device=frames.device)
            spans = torch.empty(1, self.time_masks, 2, dtype=torch.int32, device=frames.device)
        L.check(lib.avllm_clip_preproc_aug(L.ptr(plan), L.ptr(frames), N, H, W, resize, image, int(clip), int(self.random_crop), self.flip_prob,
                                           self.time_masks, self.time_width, self.time_ratio, self.fill, int(seed) & 0xFFFFFFFF,
                                           self._seed_ptr(seed_dev), L.ptr(out), L.dt_of(out), L.ptr(info), L.ptr(spans) if self.time_masks else None,
                                           L.ptr(self._ws), self._ws.numel(), L.stream_ptr()))
        if own:
            self.last_info, self.last_spans, self.last_frames = info, spans, [N]
        return out

    def pixels(self, video, nframes=None, seed=0, first_clip=0, seed_dev=None):
        """Flip and frame masks IN PLACE on pixel_values [B, F, 3, S, S] (contiguous float32 / bfloat16 on the device) that were resized and
        cropped before; nframes int32 [B] on the device | None (= F): the frames each clip really has.  Clip b draws with the keys of clip
        first_clip + b.  Returns video.  With flip_prob rounding to 0 and no masks nothing is launched."""
        if video.dim() != 5 or video.shape[2] != 3 or video.shape[3] != video.shape[4] or not video.is_contiguous() or not video.is_cuda:
            raise ValueError(f"VideoAugment.pixels: video should be a contiguous [batch_size, frames, 3, size, size] device tensor, got {tuple(video.shape)}")
        B, F, _, S, _ = video.shape
        if nframes is not None and (nframes.dtype != torch.int32 or tuple(nframes.shape) != (B,) or not nframes.is_contiguous() or nframes.device != video.device):
            raise ValueError(f"VideoAugment.pixels: nframes should be a contiguous int32 [{B}] tensor on {video.device}, got {nframes.dtype} {tuple(nframes.shape)} on {nframes.device}")
        if int(first_clip) < 0:
            raise ValueError(f"VideoAugment.pixels: first_clip = {first_clip} may not be negative")
        info = torch.empty(B, 4, dtype=torch.int32, device=video.device)
        spans = torch.empty(B, self.time_masks, 2, dtype=torch.int32, device=video.device)
        if int(C.c_float(self.flip_prob).value * 16777216.0 + 0.5) == 0 and self.time_masks == 0:      # no launch: the draw it would have left
            info[:, :2], info[:, 2:] = -1, 0
        L.check(L.load().avllm_video_frames_augment(L.ptr(video), L.dt_of(video), B, F, S, L.ptr(nframes), int(first_clip), self.flip_prob,
                                                    self.time_masks, self.time_width, self.time_ratio, self.fill, int(seed) & 0xFFFFFFFF,
                                                    self._seed_ptr(seed_dev), L.ptr(info), L.ptr(spans) if self.time_masks else None,
                                                    L.stream_ptr()))
        self.last_info, self.last_spans, self.last_frames = info, spans, nframes if nframes is not None else [F] * B
        return video

    @staticmethod
    def info_fields(info):
        """last_info (int32 [clips, 4], on any device) -> dict of host lists: left, top, flip, masked."""
        info = info.cpu()
        return {"left": info[:, 0].tolist(), "top": info[:, 1].tolist(), "flip": info[:, 2].tolist(), "masked": info[:, 3].tolist()}


def video_augment_from_config(cfg):
    """The VideoAugment the flat configuration asks for (keys video_resize, video_random_crop, video_flip_prob, video_time_masks,
    video_time_width, video_time_ratio: scripts/clip_whisper/train.py flags and configs/clip_whisper.yaml data: entries), or None when it asks
    for none: the trainer then runs exactly the path it ran without these keys.  A resize asks for the random crop unless video_random_crop
    says otherwise; flip and masks are off until asked for."""
    resize, crop, flip = cfg.get("video_resize"), cfg.get("video_random_crop"), cfg.get("video_flip_prob")
    tm = int(cfg.get("video_time_masks") or 0)
    if isinstance(crop, str):
        crop = crop.strip().lower() in ("1", "true", "yes", "on")
    if resize is None and not flip and tm == 0:      # without a resize there is no room to crop: video_random_crop alone asks for nothing
        return None
    return VideoAugment(resize=None if resize is None else int(resize), random_crop=resize is not None if crop is None else bool(crop),
                        flip_prob=float(flip or 0.0), time_masks=tm, time_width=int(cfg.get("video_time_width") or 0),
                        time_ratio=1.0 if cfg.get("video_time_ratio") is None else float(cfg.get("video_time_ratio")))


def parse_snr(value):
    """--noise_snr / the YAML's noise_snr: "LO,HI", [LO, HI], or one number -> (lo, hi)."""
    if isinstance(value, str):
        value = [float(t) for t in value.split(",")]
    if isinstance(value, (int, float)):
        value = [value]
    if len(value) not in (1, 2):
        raise ValueError(f"noise_snr: one value or LO,HI expected, got {value}")
    return float(value[0]), float(value[-1])


def augment_from_config(cfg, device):
    """The AudioAugment the flat configuration asks for (keys noise_path, noise_snr, noise_prob, spec_time_masks, spec_time_width,
    spec_time_ratio, spec_freq_masks, spec_freq_width: scripts/clip_whisper/train.py flags and configs/clip_whisper.yaml data: entries), or None
    when it asks for none: the trainer then runs exactly the path it ran without these keys."""
    path = cfg.get("noise_path")
    tm, fm = int(cfg.get("spec_time_masks") or 0), int(cfg.get("spec_freq_masks") or 0)
    if not path and tm + fm == 0:
        return None
    snr = parse_snr(cfg.get("noise_snr") if cfg.get("noise_snr") is not None else (0.0, 20.0))
    prob = cfg.get("noise_prob")
    return AudioAugment(noise=NoiseBank(path, device) if path else None, snr_db=snr, noise_prob=1.0 if prob is None else float(prob),
                        time_masks=tm, time_width=int(cfg.get("spec_time_width") or 0),
                        time_ratio=1.0 if cfg.get("spec_time_ratio") is None else float(cfg.get("spec_time_ratio")),
                        freq_masks=fm, freq_width=int(cfg.get("spec_freq_width") or 0))


def valid_frames(lengths):
    """The log-mel frames a clip of `lengths` samples really has: min(3000, ceil(len / 160)) (hop 160), int32 like its input."""
    return torch.clamp((lengths + 159) // 160, max=N_FRAMES).to(torch.int32)


def device_collate(samples, logmel, clip_frames, max_video_length=300, augment=None, seed=None, video_augment=None):
    """collate_fn (simple_dataset.py:317-460) for raw samples: `samples` = list of dicts with "wave" (1-D float, 16 kHz) and/or
    "frames" (uint8 [F,H,W,3]) + "labels"/"text".  -> (audio [B,80,3000] | None, video [B,Fmax,3,S,S] zero-padded | None).
    augment: an AudioAugment | None; with one, noise is mixed into the padded waveforms (in place, over each clip's own samples) before the
    log-mel and the features are masked after it, both drawn with `seed`.  None: the calls and allocations of before.
    video_augment: a VideoAugment | None; with one, each clip's frames take the fused resize / crop / flip / mask path, the sample's index in the
    batch as its `clip`, drawn with `seed` too (a salt of its own keeps the two streams' draws apart).  None: the calls of before."""
    audio = video = None
    if (augment is not None or video_augment is not None) and seed is None:
        raise ValueError("device_collate: augment needs a seed (the draws of a batch are a function of it)")
    if all(s.get("wave") is not None for s in samples):
        if augment is not None:
            wave, lengths = logmel.pad_batch([s["wave"] for s in samples], return_lengths=True)
            audio = logmel(augment.wave(wave, lengths, seed, out=wave))
            if augment.masks:
                augment.features(audio, valid_frames(lengths), seed)
        else:
            audio = logmel([s["wave"] for s in samples])
    if all(s.get("frames") is not None for s in samples):
        if video_augment is not None:
            va, dev = video_augment, clip_frames.device
            info = torch.empty(len(samples), 4, dtype=torch.int32, device=dev)
            spans = torch.empty(len(samples), va.time_masks, 2, dtype=torch.int32, device=dev)
            clips = [va.frames(clip_frames, torch.as_tensor(s["frames"])[:max_video_length], i, seed, info=info[i], spans=spans[i])
                     for i, s in enumerate(samples)]
            va.last_info, va.last_spans, va.last_frames = info, spans, [c.shape[0] for c in clips]
        else:
            clips = [clip_frames(torch.as_tensor(s["frames"])[:max_video_length]) for s in samples]
        Fmax = max(c.shape[0] for c in clips)
        video = torch.zeros(len(clips), Fmax, *clips[0].shape[1:], dtype=clips[0].dtype, device=clips[0].device)
        for i, c in enumerate(clips):
            video[i, : c.shape[0]] = c
    return audio, video
