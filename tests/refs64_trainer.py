"""A host restatement of ONE optimizer step of avllm.trainer.ClipWhisperTrainer, from a window's micro-batches to the updated parameters, built
only from what the suite already pins:
  the augmentation seed          refs64_augment.augment_seed at the micro-batch's index (one per micro-batch handed to train_step)
  the augmented inputs           refs64_augment.add_noise / spec_augment, refs_video_augment.augment_clip / pixels_augment, oracle.preprocess
  the modes                      refs64_modality.draw at the step's seed (refs64.dropout_seed) plus micro * AVLLM_MICRO_SEED_STRIDE
  the LoRA dropout masks         refs64_gemm.keep_grid at seed + 4 * layer + module over the [B * S, d] rows, times refs64_gemm.drop_scale
  loss and gradients             connector_expect.connector_step(modes=, dtype=float64): the oracle's functions, refs64_modality's fusion
  the window                     SUM cross entropy and gradient sums over the micro-batches, divided by the window's scored tokens; one global
                                 norm over connectors + LoRA, one clip coefficient, refs64.adamw_step under refs64.schedule; a non-finite
                                 window touches nothing and advances neither the schedule nor the bias corrections (skipped += 1)
Parameters, gradients and moments are dicts: "lora.<layers.N.module.lora_A|B>" and the four connector keys of connector_expect.
float64 wherever connector_step runs float64 (its docstring says what stays fp32).

`wrong` plants defects (DEFECTS below); tests/test_trainer_cases_cpu.py shows that the comparison of tests/trainer_cases.py catches each."""
import math
from types import SimpleNamespace

import numpy as np
import torch

import connector_expect as CE
import refs64 as R
import refs64_augment as RA
import refs64_gemm as RG
import refs64_modality as RM
import refs_video_augment as RV
from oracle import preprocess as P

M32 = 0xFFFFFFFF
MICRO_SEED_STRIDE = 0xC2B2AE35                     # include/avllm.h AVLLM_MICRO_SEED_STRIDE (tests/test_grad_accum_host_cpu.py reads it from the header)
LORA_MODULES = ("q_proj", "k_proj", "v_proj", "o_proj")

DEFECTS = ("shared_aug_seed", "modes_prev_seed", "modes_frozen", "dropped_stream_grad", "div_by_N", "clip_per_micro", "norm_lora_only",
           "shared_salt", "augment_validation", "skip_advances_schedule", "decay_biases", "resume_from_zero", "lr_at_step_plus_skipped",
           "schedule_args_swapped")


def micro_seed(step, skipped, micro, rank=0):
    """avllm_step_advance_micro: the step's seed plus micro * AVLLM_MICRO_SEED_STRIDE; micro-step 0 (and grad_accum_steps = 1) keeps the step's."""
    return (R.dropout_seed(step, skipped, rank=rank) + micro * MICRO_SEED_STRIDE) & M32


def lora_masks(layers, hidden, seed, B, S, p):
    """The masks of avllm_llama_lora_fwd_loss for the four attention adapters, already scaled by 1 / (1 - p): {`layers.N.module`: [B, S, d]}."""
    scale = RG.drop_scale(p)
    return {f"layers.{l}.{nm}": (RG.keep_grid((seed + 4 * l + j) & M32, B * S, hidden, hidden, p).double() * scale).view(B, S, hidden)
            for l in range(layers) for j, nm in enumerate(LORA_MODULES)}


# ---------------------------------------------------------------- the inputs of a micro-batch
_FEATS, _RESIZED, _PLAIN = {}, {}, {}


def _valid(n):
    return min(3000, -(-n // 160))


def augmented_inputs(c, mb, seed, training=True, wrong=()):
    """What _unpack hands to train_step for micro-batch `mb` under the augmentation seed `seed` -> (audio float32 [B, M, 3000], video float32
    [B, F, 3, S, S], info).  mb["form"]: "raw" (mb["samples"]: dicts with "wave", "frames" and an "id" for the caches) or tensors (mb["audio"],
    mb["video"]).  An eval-mode batch (training=False) is not augmented.  info: the noise draws, the SpecAugment spans, the video draws."""
    on = training or "augment_validation" in wrong
    aa, va = (c.audio_aug, c.video_aug) if on else (None, None)
    info = {"noise": None, "spans": None, "video": None}
    saved = RV.video_draw
    if "shared_salt" in wrong:
        RV.video_draw = lambda *a, **k: saved(*a, **dict(k, salt=RA.SPEC_SALT))
    try:
        if mb["form"] == "raw":
            samples = mb["samples"]
            waves = [np.asarray(s["wave"], dtype=np.float32) for s in samples]
            lengths = [len(w) for w in waves]
            mixed = False
            if aa is not None and aa.get("noise") is not None:
                padded = np.zeros((len(waves), max(lengths)), dtype=np.float32)
                for b, w in enumerate(waves):
                    padded[b, : len(w)] = w
                lo, hi = aa["snr_db"]
                out, info["noise"] = RA.add_noise(padded, lengths, aa["noise"], seed, aa["noise_prob"], None, lo, hi)
                waves, mixed = [out[b, :n] for b, n in enumerate(lengths)], True
            feats = []
            for s, w, i in zip(samples, waves, info["noise"] or [None] * len(waves)):
                if mixed and i["applied"]:
                    feats.append(P.audio_features(w))
                else:
                    if s["id"] not in _FEATS:
                        _FEATS[s["id"]] = P.audio_features(w)
                    feats.append(_FEATS[s["id"]])
            audio = np.stack(feats).astype(np.float32)
            if aa is not None and aa["time_masks"] + aa["freq_masks"] > 0:
                audio, info["spans"] = RA.spec_augment(audio, [_valid(n) for n in lengths], seed, aa["time_masks"], aa["time_width"], aa["time_ratio"],
                                                       aa["freq_masks"], aa["freq_width"], aa["fill"])
            S = c.image
            clips, draws = [], []
            for i, s in enumerate(samples):
                if va is not None:
                    resize = va["resize"] or S
                    key = (s["id"], resize)
                    if key not in _RESIZED:
                        _RESIZED[key] = RV.resize_clip(s["frames"], resize)
                    out, d = RV.augment_clip(s["frames"], i, seed, resize, S, va["random_crop"], va["flip_prob"], va["time_masks"], va["time_width"],
                                             va["time_ratio"], va["fill"], resized=_RESIZED[key])
                    draws.append(d)
                else:
                    if s["id"] not in _PLAIN:
                        _PLAIN[s["id"]] = np.stack([P.clip_pixel_values(f, S) for f in s["frames"]]).astype(np.float32)
                    out = _PLAIN[s["id"]]
                clips.append(out)
            video = np.zeros((len(clips), max(len(x) for x in clips), 3, S, S), dtype=np.float32)
            for i, x in enumerate(clips):
                video[i, : len(x)] = x
            info["video"] = draws or None
        else:
            audio = mb["audio"].numpy()
            if aa is not None and aa["time_masks"] + aa["freq_masks"] > 0:
                audio, info["spans"] = RA.spec_augment(audio, None, seed, aa["time_masks"], aa["time_width"], aa["time_ratio"], aa["freq_masks"],
                                                       aa["freq_width"], aa["fill"])
            video = mb["video"].numpy()
            if va is not None:
                video, info["video"] = RV.pixels_augment(video, None, seed, 0, va["flip_prob"], va["time_masks"], va["time_width"], va["time_ratio"],
                                                         np.float32(va["fill"]))
    finally:
        RV.video_draw = saved
    return torch.from_numpy(np.ascontiguousarray(audio)), torch.from_numpy(np.ascontiguousarray(video)), info


# ---------------------------------------------------------------- clip + AdamW + schedule
def trainable(c, par):
    return [k for k in par if k.startswith("lora.") or c.conn]


def apply_rule(c, before, grads, finite, wrong=(), sched=None, micro_grads=None, dtype=torch.float64, coef=None, abi=False):
    """One global norm over the trainable tensors, one clip coefficient, AdamW (connector biases not decayed) under the cosine schedule, on
    copies of before.par / .mo / .vo in `dtype` -> SimpleNamespace(par, mo, vo, step, skipped, coef).  A non-finite window: copies of what was,
    the same step count, skipped one higher.  sched: the (lr, bc1, bc2_sqrt) to use instead of refs64.schedule's (a device's own record).
    coef: the factor to put on `grads` instead of the clip coefficient of their own norm (a device's: from its own sum of squares, and with
    grad_accum_steps > 1 on its gradient SUMS, the prescale 1 / count included).  abi: the constants as the kernel's float arguments hold them
    (beta1, beta2, eps, the weight decay: refs64_augment.as_f32), so that 1 - beta1 is the kernel's 1.0f - beta1."""
    h = c.hyper
    par, mo, vo = ({k: v.to(dtype).clone() for k, v in d.items()} for d in (before.par, before.mo, before.vo))
    if not finite:
        return SimpleNamespace(par=par, mo=mo, vo=vo, step=before.step + (1 if "skip_advances_schedule" in wrong else 0), skipped=before.skipped + 1,
                               coef=None)
    step = before.step + 1
    keys = trainable(c, par)
    g = {k: grads[k].to(dtype) for k in keys}
    normed = [k for k in keys if k.startswith("lora.")] if "norm_lora_only" in wrong else keys
    if coef is None:
        coef = R.clip_coef(math.fsum(float((g[k].double() ** 2).sum()) for k in normed), h.grad_clip)
    if "clip_per_micro" in wrong and micro_grads is not None:
        g = {k: torch.zeros_like(g[k]) for k in keys}
        for part in micro_grads:
            ci = R.clip_coef(math.fsum(float((part[k].double() ** 2).sum()) for k in keys), h.grad_clip)
            for k in keys:
                g[k] += ci * part[k].to(dtype)
        coef = 1.0
    lr, bc1, bc2s = R.schedule(step, h.lr, h.total_steps, h.warmup_steps) if sched is None else sched
    f = RA.as_f32 if abi else float
    for k in keys:
        wd = 0.0 if (k.endswith("bias") and "decay_biases" not in wrong) else h.weight_decay
        R.adamw_step(par[k], g[k], mo[k], vo[k], lr, step, coef=coef, b1=f(0.9), b2=f(0.95), eps=f(1e-8), wd=f(wd), bc1=bc1, bc2_sqrt=bc2s)
    return SimpleNamespace(par=par, mo=mo, vo=vo, step=step, skipped=before.skipped, coef=coef)


def clip_coef32(sumsq, max_norm, prescale=1.0):
    """refs64.clip_coef with every operation in float32, in the kernel's order: prescale * min(1, max_norm / (sqrt(sumsq) * prescale + 1e-6)).
    What "the same rule in fp32 on the host" uses when bars.fp32_bar measures the reachable accuracy of an optimizer step from its inputs."""
    f = np.float32
    coef = f(prescale)
    if max_norm > 0:
        coef = coef * np.minimum(f(1.0), f(max_norm) / (np.sqrt(f(sumsq)) * f(prescale) + f(1e-6)))
    return float(f(coef))


def weights_of(W, c, par):
    """The oracle's weight dict with the LoRA tensors (and, when they train, the connectors) taken from `par`."""
    Wn = dict(W)
    Wn["lora"] = {k[5:]: v for k, v in par.items() if k.startswith("lora.")}
    if c.conn:
        for name in ("audio_connector", "video_connector"):
            Wn[name] = {k: par[f"{name}.{k}"] for k in W[name]}
    return Wn


def scored(labels, pad):
    return int((labels[:, 1:] != pad).sum())


def step(c, W, oc, before, micro, aug_index, rank0=0, wrong=(), dtype=torch.float64):
    """One optimizer step on the window `micro` (a list of micro-batches: augmented_inputs' `mb` plus "labels" [B, S] and "prompt" [B, P] ids;
    under data parallelism the micro-batches of every rank, each with its "rank" and its position "micro" in that rank's window).
    before: SimpleNamespace(par, mo, vo, step, skipped) -- the parameters and moments and the DEVICE-side counts of steps taken and skipped.
    aug_index: the augmentation index of the window's first micro-batch.
    -> SimpleNamespace(modes [per micro-batch: list | None], inputs [(audio, video)], infos, loss, finite, grads (pre-clip, of the window's
    token-mean loss), counts, par, mo, vo, step, skipped, lr, bc1, bc2_sqrt)."""
    h = c.hyper
    wrong = set(wrong)
    step_no = before.step + 1
    Wn = weights_of(W, c, before.par)
    keys = [k for k in before.par]
    loss_sum, counts, modes_all, inputs, infos, micro_grads = 0.0, [], [], [], [], []
    for pos, mb in enumerate(micro):
        j, rank = mb.get("micro", pos), mb.get("rank", rank0)        # data parallel: a rank's micro-batches carry its number and their position
        idx = (0 if "resume_from_zero" in wrong else aug_index) + (0 if "shared_aug_seed" in wrong else j)
        audio, video, info = augmented_inputs(c, mb, RA.augment_seed(h.augment_seed, idx, rank), True, wrong)
        labels, prompt = mb["labels"], mb["prompt"]
        B, S = labels.shape
        base = micro_seed(step_no, before.skipped, j, rank)
        modes = None
        if c.moddrop is not None:
            s = base
            if "modes_prev_seed" in wrong:
                s = micro_seed(step_no - 1, before.skipped, j, rank)
            if "modes_frozen" in wrong:
                s = micro_seed(1, 0, 0, rank)
            modes = RM.draw(B, c.moddrop[0], c.moddrop[1], s)
        masks = lora_masks(oc.llama.layers, oc.llama.hidden, base, B, S, c.drop) if c.drop else None
        loss, _, cg, lg = CE.connector_step(Wn, oc, audio, video, prompt, labels, masks=masks, modes=modes, dtype=dtype, wrong=wrong)
        n = scored(labels, oc.pad_token_id)
        g = {"lora." + k: v for k, v in lg.items()}
        g.update(cg)
        loss_sum += float(loss) * n
        counts.append(n)
        micro_grads.append({k: g[k].double() * n for k in keys})
        modes_all.append(modes)
        inputs.append((audio, video))
        infos.append(info)
    count = sum(counts)
    loss = loss_sum / count
    finite = math.isfinite(loss)
    div = float(sum(counts)) if "div_by_N" not in wrong else None
    grads = {}
    for k in keys:
        if div is None:                                          # the mean of the micro-batches' mean gradients
            grads[k] = sum(part[k] / n for part, n in zip(micro_grads, counts)) / len(micro)
        else:
            grads[k] = sum(part[k] for part in micro_grads) / div
    # the schedule record of the step: a function of the count of steps TAKEN alone (a skipped step is tried again under its own number)
    sched_step = step_no + (before.skipped if "lr_at_step_plus_skipped" in wrong else 0)
    total, warm = (h.warmup_steps, h.total_steps) if "schedule_args_swapped" in wrong else (h.total_steps, h.warmup_steps)
    lr, bc1, bc2s = R.schedule(sched_step, h.lr, total, warm)
    after = apply_rule(c, before, grads, finite, wrong, sched=(lr, bc1, bc2s), micro_grads=[{k: v / count for k, v in part.items()} for part in micro_grads])
    return SimpleNamespace(modes=modes_all, inputs=inputs, infos=infos, loss=loss, finite=finite, grads=grads, counts=counts, par=after.par,
                           mo=after.mo, vo=after.vo, step=after.step, skipped=after.skipped, lr=lr, bc1=bc1, bc2_sqrt=bc2s, coef=after.coef)
