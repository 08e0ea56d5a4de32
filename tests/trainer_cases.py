"""ClipWhisperTrainer.train_step() across pairings of trainer forms: the case table, which trainer paths a case takes, the data and the call
sequence of a case, and the comparison of one optimizer step with tests/refs64_trainer.py.  Pure CPU, everything from seeds:
tests/test_trainer_cases_cpu.py checks the table and the restatement on the host, tests/test_trainer_matrix_gpu.py runs every case on the trainer.

Twelve factors are the settings avllm/trainer.py branches on.  CASES is an explicit list that holds every pair of levels of every two factors
at least once, except the pairs the code cannot take (IMPOSSIBLE), and starts with the default deployment and a case with everything on.
A case is 3 optimizer steps (4 with grad_accum_steps = 1, so that a captured signature is also replayed) on the tiny golden model
(oracle.weights.tiny()): micro-batches of 3 clips (signature A) or 2 clips (signature B) out of a pool of 6, 3 to 5 frames per clip, labels of 24
tokens with uneven scored counts, raw waves of 0.5 to 2 s and raw frames of 40 x 56 on a CLIP image of 48, a noise bank of three recordings."""
import itertools
import math
from types import SimpleNamespace

import numpy as np
import torch

import bars as Bar
import refs64 as R
import refs64_trainer as RT

FACTORS = {"accum": ("1", "2", "3f"),                     # grad_accum_steps 1; 2; 3 with a last window of 2 closed by flush()
           "launch": ("eager", "graph"),
           "conn": (0, 1),                                # train_connectors
           "precision": ("fp32", "bf16"),
           "drop": (0.0, 0.05),                           # lora_dropout
           "moddrop": ("off", "0.3/0.3", "0.5/0"),        # modality_dropout_audio / _video
           "form": ("dict", "tuple", "raw"),              # _unpack's three input forms
           "audio": ("off", "spec", "noise+spec"),
           "video": ("off", "flip+mask", "crop+flip+mask"),
           "pieces": (1, 2),                              # bwd_pieces
           "sigs": ("one", "two"),                        # input signatures, alternating (inside a window too)
           "event": ("none", "nonfinite", "resume")}

# The pairs the code cannot take.  Neither is an exception: on a batch of tensors the trainer applies the half of the augmentation that needs no
# raw sample and logs that once, so the raw-only LEVEL does not exist for these forms (its other half is the level next to it):
#   avllm/trainer.py _augment_features ("noise needs raw waveforms": `return aug.features(audio, None, ...)`, the SpecAugment half only)
#   avllm/trainer.py _augment_pixels   ("the crop needs raw frames": `aug.pixels(video, None, ...)`, flip and frame masks only)
IMPOSSIBLE = tuple(("form", f, fac, lv) for f in ("dict", "tuple") for fac, lv in (("audio", "noise+spec"), ("video", "crop+flip+mask")))

# name, then the levels in the order of FACTORS.  The first is the default deployment (N = 1, graph, LoRA only, bf16, dropout 0.05, nothing else
# on), the second has everything on; c02 .. c14 complete the pairs (a greedy search, then written out); raw-plain is device_collate without
# augmenters, which no pair asks for.
_TABLE = (
    ("default-deployment", "1", "graph", 0, "bf16", 0.05, "off", "dict", "off", "off", 1, "one", "none"),
    ("everything-on", "3f", "graph", 1, "fp32", 0.05, "0.3/0.3", "raw", "noise+spec", "crop+flip+mask", 2, "two", "resume"),
    ("c02", "3f", "eager", 0, "bf16", 0.0, "0.5/0", "tuple", "spec", "flip+mask", 2, "one", "nonfinite"),
    ("c03", "2", "eager", 1, "fp32", 0.0, "off", "dict", "off", "off", 1, "two", "resume"),
    ("c04", "1", "eager", 1, "fp32", 0.0, "0.5/0", "raw", "noise+spec", "flip+mask", 1, "one", "none"),
    ("c05", "2", "graph", 0, "bf16", 0.05, "off", "raw", "noise+spec", "crop+flip+mask", 2, "one", "nonfinite"),
    ("c06", "2", "eager", 1, "bf16", 0.05, "0.3/0.3", "tuple", "spec", "off", 1, "two", "none"),
    ("c07", "3f", "graph", 0, "fp32", 0.05, "0.5/0", "dict", "spec", "flip+mask", 1, "two", "resume"),
    ("c08", "1", "graph", 1, "bf16", 0.0, "0.3/0.3", "tuple", "off", "flip+mask", 2, "two", "resume"),
    ("c09", "3f", "eager", 1, "fp32", 0.0, "off", "tuple", "off", "off", 2, "two", "nonfinite"),
    ("c10", "1", "eager", 1, "fp32", 0.05, "0.3/0.3", "raw", "spec", "crop+flip+mask", 1, "one", "nonfinite"),
    ("c11", "3f", "graph", 1, "fp32", 0.0, "0.5/0", "raw", "off", "crop+flip+mask", 2, "one", "none"),
    ("c12", "2", "eager", 0, "bf16", 0.05, "0.3/0.3", "dict", "spec", "flip+mask", 2, "one", "nonfinite"),
    ("c13", "2", "eager", 0, "bf16", 0.05, "0.5/0", "raw", "noise+spec", "off", 2, "one", "resume"),
    ("c14", "3f", "graph", 0, "bf16", 0.05, "off", "raw", "spec", "flip+mask", 1, "one", "nonfinite"),
    ("raw-plain", "2", "graph", 1, "fp32", 0.05, "off", "raw", "off", "off", 1, "two", "none"),
    # beyond the pairs, two events in one case: the checkpoint is written after a skipped window, so the resumed trainer starts from skipped = 1,
    # which is part of every later step's dropout and modality seed
    ("skip-then-resume", "2", "eager", 1, "fp32", 0.05, "0.3/0.3", "dict", "spec", "off", 1, "one", "nonfinite+resume"),
)

HYPER = dict(lr=1e-3, total_steps=10, warmup_steps=0, grad_clip=0.5, weight_decay=0.01, augment_seed=9)
# the cases that run under a linear warm-up of 2 steps (no pair asks for it; the schedule record of every step is compared either way): two with
# a non-finite window, two that resume, in both precisions
WARMUP = {"c03": 2, "c05": 2, "c08": 2, "c09": 2}
IMAGE, FRAME_HW, CROP_RESIZE = 48, (40, 56), 56
SPEC = dict(time_masks=2, time_width=20, time_ratio=0.5, freq_masks=2, freq_width=9, fill=0.0)
NOISE = dict(snr_db=(0.0, 10.0), noise_prob=0.75)
VIDEO = dict(flip_prob=0.5, time_masks=2, time_width=2, time_ratio=0.6, fill=0.0)
LOGMEL_ABS = 2e-5                                        # tests/test_preprocess_gpu.py: the device log-mel against oracle.preprocess


def _case(name, *levels):
    c = SimpleNamespace(name=name, **dict(zip(FACTORS, levels)))
    c.N = {"1": 1, "2": 2, "3f": 3}[c.accum]
    c.graph = c.launch == "graph"
    c.moddrop = None if c.moddrop == "off" else tuple(float(x) for x in c.moddrop.split("/"))
    c.levels = dict(zip(FACTORS, levels))
    c.hyper, c.image = SimpleNamespace(**dict(HYPER, warmup_steps=WARMUP.get(name, 0))), IMAGE
    c.audio_aug = None if c.audio == "off" else dict(SPEC, noise=noise_rows() if c.audio == "noise+spec" else None, **NOISE)
    c.video_aug = None if c.video == "off" else dict(VIDEO, resize=CROP_RESIZE if c.video.startswith("crop") else None, random_crop=c.video.startswith("crop"))
    return c


def noise_rows():
    """The noise bank, kept in memory: three recordings of 3000, 9000 and 777 samples."""
    g = np.random.default_rng(7)
    return [(0.2 * g.standard_normal(n)).astype(np.float32) for n in (3000, 9000, 777)]


CASES = [_case(*row) for row in _TABLE]
BY_NAME = {c.name: c for c in CASES}


def missing_pairs(cases=None):
    """The (factor, level, factor, level) pairs no case of the list holds, the IMPOSSIBLE ones left out."""
    want = {(fa, a, fb, b) for fa, fb in itertools.combinations(FACTORS, 2) for a in FACTORS[fa] for b in FACTORS[fb]} - set(IMPOSSIBLE)
    for c in CASES if cases is None else cases:
        want -= {(fa, c.levels[fa], fb, c.levels[fb]) for fa, fb in itertools.combinations(FACTORS, 2)}
    return sorted(want, key=str)


def forms(c):
    """Which paths of avllm/trainer.py case c takes, restated from its branches."""
    tensors = c.form in ("dict", "tuple")
    return {
        "_eager_step": c.N == 1,                                   # train_step: N == 1; the first two visits of a signature are eager with graphs too
        "_replay": c.N == 1 and c.graph,                           # the third visit of a signature on
        "_micro_train_step": c.N > 1,
        "_replay_micro": c.N > 1 and c.graph,
        "_close_graph": c.N > 1 and c.graph,                       # _close_window: warm -> capture -> replay
        "_part_opt_connectors": c.N == 1 and bool(c.conn),         # _part_opt's branch
        "_part_close": c.N > 1,
        "_part_close(connectors)": c.N > 1 and bool(c.conn),       # its adamw_step_multi branch
        "_augment_features": tensors and c.audio != "off",
        "_augment_pixels": tensors and c.video != "off",
        "device_collate(augmenters)": c.form == "raw" and (c.audio != "off" or c.video != "off"),
        "device_collate(plain)": c.form == "raw" and c.audio == "off" and c.video == "off",
        "tokenizer": c.form != "dict",                             # the prompt from texts
        "modality_draw": c.moddrop is not None,
        "pieces_split": c.pieces == 2,                             # _piece_range with two pieces; the connector backward follows the second
        "deferred_save": "resume" in c.event and c.N > 1,          # _save_checkpoint asked for mid-window
        "load_checkpoint": "resume" in c.event,
        "flush": c.accum == "3f",
    }


# ---------------------------------------------------------------- the data of the cases
_POOL = {}
TEXTS = ("ab cd", "hello", "the quick brown", "a longer prompt text", "mid size", "xy")        # clip 2 is the longest of A, clip 3 of B
WAVE_SAMPLES = (16000, 8000, 24000, 32000, 12000, 20000)
FRAME_COUNTS = (4, 3, 5, 5, 4, 3)
# every A holds clip 2 and not clip 3, every B clip 3 (the longest text, 5 frames): one prompt width and one frame count per signature; the clips
# around them change, so that the micro-batches of a window hold different numbers of scored tokens
SIG = {"A": ((0, 1, 2), (2, 4, 1), (5, 2, 0), (1, 2, 5), (4, 2, 0)), "B": ((3, 4), (5, 3), (3, 0), (1, 3))}


def pool():
    """(oc, W, audio [6, 80, 3000], video [6, 5, 3, 48, 48] (clip 1: 3 frames, zero-padded as device_collate pads), labels [6, 24], prompt [6, 32],
    raw samples).  Labels: clips 0, 3 and 4 end early, so micro-batches hold different numbers of scored tokens."""
    if not _POOL:
        from oracle import weights as Wt
        from oracle.make_golden_preproc import frame_case, wave_case
        oc = Wt.tiny()
        W = Wt.all_weights(oc, 0, lora_b_std=0.05)
        audio, video, labels, prompt = Wt.synthetic_batch(oc, 6, 5, seed=77)
        labels = labels[:, :24].contiguous()
        labels[0, 12:], labels[3, 9:], labels[4, 16:] = oc.pad_token_id, oc.pad_token_id, oc.pad_token_id
        video = video.clone()
        video[1, 3:] = 0.0
        raw = [{"id": i, "wave": wave_case(21 + i, n), "frames": np.stack([frame_case(30 + 10 * i + j, *FRAME_HW) for j in range(f)])}
               for i, (n, f) in enumerate(zip(WAVE_SAMPLES, FRAME_COUNTS))]
        _POOL["pool"] = (oc, W, audio, video, labels, prompt, raw)
    return _POOL["pool"]


def schedule(c):
    """The case's windows: a list of optimizer steps, each a list of (clip indices, poisoned) micro-batches.  The last window of a "3f" case
    holds 2 micro-batches and is closed by flush().  event "nonfinite": the last micro-batch of the second window is poisoned."""
    two = c.sigs == "two"
    if c.N == 1:
        windows = [["A"], ["B"], ["A"], ["A"]] if two else [["A"]] * 4      # A: warm, capture, replay; B runs eager among them
    elif c.N == 2:
        windows = [["A", "B" if two else "A"]] * 3
    else:
        windows = [["A", "B" if two else "A", "A"]] * 2 + [["A", "B" if two else "A"]]
    it = {k: itertools.cycle(v) for k, v in SIG.items()}
    out = [[(next(it[s]), False) for s in w] for w in windows]
    if "nonfinite" in c.event:
        out[1][-1] = (out[1][-1][0], True)
    return out


def prompt_ids(idx):
    from avllm.tokenizer import ByteTokenizer
    return ByteTokenizer(256)([TEXTS[i] for i in idx], return_tensors="pt", padding=True, truncation=True, max_length=512).input_ids


def _poisoned_sample(s):
    w = s["wave"].copy()
    w[0] = np.nan
    return dict(s, wave=w, id=("nan", s["id"]))


def host_batch(c, idx, poisoned=False):
    """The micro-batch as tests/refs64_trainer.py takes it.  Poisoned: a NaN in every clip's audio (and, in a tensor, its video), so that whatever
    modes are drawn the loss is not finite."""
    oc, W, audio, video, labels, prompt, raw = pool()
    idx = list(idx)
    mb = {"form": c.form, "labels": labels[idx], "prompt": prompt[idx] if c.form == "dict" else prompt_ids(idx)}
    if c.form == "raw":
        mb["samples"] = [_poisoned_sample(raw[i]) if poisoned else raw[i] for i in idx]
    else:
        mb["audio"], mb["video"] = audio[idx].clone(), video[idx].clone()
        if poisoned:
            mb["audio"][:, 0, 0] = float("nan")
            mb["video"][:, 0, 0, 0, 0] = float("nan")
    return mb


def trainer_batch(c, idx, poisoned=False, device="cuda"):
    """The same micro-batch as the trainer's _unpack takes it: a dict of tensors, the (audio, video, texts, labels) tuple, or raw samples."""
    mb = host_batch(c, idx, poisoned)
    texts = [TEXTS[i] for i in idx]
    if c.form == "raw":
        return {"raw": [{"wave": s["wave"], "frames": s["frames"]} for s in mb["samples"]], "texts": texts, "labels": mb["labels"].to(device)}
    a, v, lab = mb["audio"].to(device), mb["video"].to(device), mb["labels"].to(device)
    if c.form == "dict":
        return {"audio": a, "video": v, "labels": lab, "prompt": mb["prompt"].to(device)}
    return (a, v, texts, lab)


def initial(c, W=None):
    """The parameters and zero moments a fresh trainer starts from, as tests/refs64_trainer.py's dicts, and the counts (0 steps, 0 skipped)."""
    import connector_expect as CE
    W = pool()[1] if W is None else W
    par = {"lora." + k: v.double().clone() for k, v in W["lora"].items()}
    if c.conn:
        par.update({k: W[k.split(".")[0]][k.split(".", 1)[1]].double().clone() for k in CE.CONNECTOR_KEYS})
    zeros = lambda: {k: torch.zeros_like(v) for k, v in par.items()}      # noqa: E731
    return SimpleNamespace(par=par, mo=zeros(), vo=zeros(), step=0, skipped=0)


# ---------------------------------------------------------------- the comparison of one optimizer step
INF = float("inf")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a), np.ascontiguousarray(b.numpy() if torch.is_tensor(b) else b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _feature_ratio(c, a, b):
    """Tensor forms: SpecAugment moves no unmasked cell, the features are compared by bits.  Raw samples: the device log-mel against
    oracle.preprocess is held to LOGMEL_ABS wherever both are finite, with NaN in the same cells, and a masked cell (the fill) by bits."""
    if c.form != "raw":
        return 0.0 if _same_bits(a, b) else INF
    a, b = a.double(), b.double()
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return INF
    fin = ~torch.isnan(b)
    return float((a[fin] - b[fin]).abs().max()) / LOGMEL_ABS if bool(fin.any()) else 0.0


def input_ratios(c, got_inputs, ref_inputs):
    """{"pixels", "features"} of lists of (audio, video): pixels bit-identical, features by _feature_ratio."""
    return {"pixels": 0.0 if all(_same_bits(g[1].float(), r[1]) for g, r in zip(got_inputs, ref_inputs)) else INF,
            "features": max(_feature_ratio(c, g[0], r[0]) for g, r in zip(got_inputs, ref_inputs))}


def ratios(c, before, got, ref):
    """Every checked quantity of one optimizer step as error / bar -> {quantity: ratio}; a quantity compared by bits is 0 or inf.
    got, ref: what refs64_trainer.step returns (got: the trainer's step read back into the same fields; ref: the restatement from `before`).
      modes      equal, for every micro-batch
      pixels     bit-identical; features: _feature_ratio
      loss       fp32 |d| / F32_LOSS_ABS, bf16 |d| / BF16_LOSS_ABS (a non-finite window: both non-finite)
      grad       the pre-clip gradient of the window's token-mean loss.  fp32: per tensor max |d| / (F32_GRAD_REL_MAX max |ref|), a tensor whose
                 reference is all zeros (the connector of a stream every clip dropped) must be all zeros; bf16: the whole LoRA gradient and the
                 whole connector gradient, relative L2 / BF16_GRAD_REL_L2
      update     parameters and both moments after the step against refs64_trainer.apply_rule in float64 on got's OWN gradient, counts and
                 schedule record, per tensor max |d| / bars.fp32_bar(float64 rule, the same rule in fp32): tests/test_bytemovers_gpu.py's AdamW bar
      sumsq      (a device's step) its sum of squares against the float64 sum over its own gradient buffers, at that file's grad_sumsq bar
      state      the counts of steps taken and skipped after the step, equal
      schedule   the step's lr, bc1 and bc2_sqrt record against refs64.schedule at the count of steps taken before it + 1, at the bar of
                 tests/test_bytemovers_gpu.py::test_step_advance (schedule_bars).  A non-finite window's record is that of the step it tried:
                 the advance writes it at the top of the step, before the guard decides, and the step tried next carries the same number
    A non-finite window has no loss / grad ratio; its update ratio is 0 when parameters and moments are bit-identical to `before`, else inf."""
    out = {}
    out["modes"] = 0.0 if [None if m is None else list(m) for m in got.modes] == [None if m is None else list(m) for m in ref.modes] else INF
    if got.inputs is not None:                                   # (two ranks: each rank compares its own batches, tests/test_trainer_matrix_gpu.py)
        out.update(input_ratios(c, got.inputs, ref.inputs))
    out["state"] = 0.0 if (got.step, got.skipped) == (ref.step, ref.skipped) else INF
    out["schedule"] = max(abs(x - y) / b for x, y, b in zip((got.lr, got.bc1, got.bc2_sqrt), (ref.lr, ref.bc1, ref.bc2_sqrt), schedule_bars(c.hyper)))
    if not ref.finite:
        same = all(_same_bits(getattr(got, f)[k].double(), getattr(before, f)[k].double()) for f in ("par", "mo", "vo") for k in before.par)
        out["update"] = 0.0 if (same and not got.finite) else INF
        return out
    if not got.finite:
        out["loss"] = INF
        return out
    f32 = c.precision == "fp32"
    out["loss"] = abs(got.loss - ref.loss) / (Bar.F32_LOSS_ABS if f32 else Bar.BF16_LOSS_ABS)
    keys = list(before.par)
    if f32:
        per = {}
        for k in keys:
            d, mx = float((got.grads[k].double() - ref.grads[k]).abs().max()), float(ref.grads[k].abs().max())
            per[k] = (0.0 if d == 0.0 else INF) if mx == 0.0 else d / (Bar.F32_GRAD_REL_MAX * mx)
        out["grad"], out["worst tensor"] = max(per.values()), max(per, key=per.get)
    else:
        for name, ks in (("grad", [k for k in keys if k.startswith("lora.")]), ("grad(connectors)", [k for k in keys if not k.startswith("lora.")])):
            if ks:
                out[name] = Bar.rel_l2(torch.cat([got.grads[k].double().flatten() for k in ks]), torch.cat([ref.grads[k].flatten() for k in ks])) / Bar.BF16_GRAD_REL_L2
    sched = (got.lr, got.bc1, got.bc2_sqrt)
    rule_g, kw, kw32 = got.grads, {}, {}
    if getattr(got, "sumsq", None) is not None:
        # a device's step: its own sum of squares is held to tests/test_bytemovers_gpu.py's bar of the fixed-order sum (bars.fp32_bar against the
        # float64 sum of its own gradient buffers, measured with torch's fp32 sum of the same) and then used, so that the update is judged on the
        # arithmetic of the rule alone; the prescale is the fp32 IEEE quotient 1 / count the kernel comment states (1 with grad_accum_steps = 1)
        rule_g = got.raw_grads
        flat = torch.cat([rule_g[k].flatten() for k in keys])
        ss64 = math.fsum((flat * flat).tolist())
        ss32 = float((flat.float() ** 2).sum())
        out["sumsq"] = abs(got.sumsq - ss64) / Bar.fp32_bar(torch.tensor([ss64], dtype=torch.float64), torch.tensor([ss32]))
        # The float64 rule takes refs64.clip_coef of that sum of squares.  Its fp32 yardstick forms the coefficient in fp32 too
        # (refs64_trainer.clip_coef32): bars.fp32_bar asks for "the same operation evaluated in fp32 on the host from the same inputs", and the
        # inputs of the optimizer launch are the sum of squares and the prescale, not a coefficient.  This is where the yardstick differs from
        # test_adamw in tests/test_bytemovers_gpu.py, which hands ONE float64 coefficient to both rules (DESIGN.md says by how much the bars
        # differ for it).  The two coefficients are held together at 8 fp32 roundings (five rounded operations -- root, product, sum,
        # quotient, product -- and room for the fp32 constant 1e-6).
        c64 = R.clip_coef(got.sumsq, c.hyper.grad_clip, got.prescale)
        c32 = RT.clip_coef32(got.sumsq, c.hyper.grad_clip, got.prescale)
        out["coef"] = abs(c32 - c64) / (8 * Bar.U32 * c64)
        kw, kw32 = dict(coef=c64, abi=True), dict(coef=c32, abi=True)
    r64 = RT.apply_rule(c, before, rule_g, True, sched=sched, **kw)
    r32 = RT.apply_rule(c, before, rule_g, True, sched=sched, dtype=torch.float32, **(kw32 or kw))
    per = {}
    for f in ("par", "mo", "vo"):
        for k in keys:
            bar = Bar.fp32_bar(getattr(r64, f)[k], getattr(r32, f)[k])
            d = float((getattr(got, f)[k].double() - getattr(r64, f)[k]).abs().max())
            per[f + " " + k] = d / bar if bar > 0.0 else (0.0 if d == 0.0 else INF)          # an all-zero tensor (a stream no clip used) stays zero
    out["update"], out["worst update"] = max(per.values()), max(per, key=per.get)
    return out


_SCHED_BARS = {}


def schedule_bars(h):
    """Bars of (lr, bc1, bc2_sqrt) as tests/test_bytemovers_gpu.py::test_step_advance forms them: 4 x the worst distance of the fp32 evaluation of
    the formula on the host (refs64.schedule(f32=True)) from float64 over the steps of this schedule (1 .. total_steps + 2), floored at 2 ulp of
    base_lr / of 1."""
    key = (h.lr, h.total_steps, h.warmup_steps)
    if key not in _SCHED_BARS:
        e32 = [0.0, 0.0, 0.0]
        for s in range(1, h.total_steps + 3):
            a, b = R.schedule(s, h.lr, h.total_steps, h.warmup_steps, f32=True), R.schedule(s, h.lr, h.total_steps, h.warmup_steps)
            e32 = [max(e, abs(x - y)) for e, x, y in zip(e32, a, b)]
        _SCHED_BARS[key] = [max(4 * e32[0], 4 * Bar.U32 * h.lr), max(4 * e32[1], 4 * Bar.U32), max(4 * e32[2], 4 * Bar.U32)]
    return _SCHED_BARS[key]


def worst(ratio):
    return max(v for v in ratio.values() if not isinstance(v, str))


def show(ratio):
    return " ".join(f"{k} {v:.3g}" if not isinstance(v, str) else f"({v})" for k, v in ratio.items())
