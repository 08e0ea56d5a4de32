"""Restatements of the acoustic augmentation kernels (csrc/augment.hip; the rules are in include/avllm.h under avllm_wave_add_noise and
avllm_spec_augment) in Python integers, numpy float64 and -- for the kernel's own float32 mix -- numpy float32: the draw, the segment with its
wrap, the energies, the gain, the mix, the spans and the masked set.  tests/test_augment_refs_cpu.py pins them to a second formulation and to
planted faults; the GPU tests compare the kernels with them under the bars of tests/bars_augment.py."""
import math
import struct

import numpy as np

from refs64_modality import M32, av_pair_hash, threshold

NOISE_SALT = 0x6E6F6973
SPEC_SALT = 0x73706563
MAX_MASKS = 32


def as_f32(x):
    """The float the C ABI receives for a Python number."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


# ---------------------------------------------------------------- avllm_wave_add_noise
def noise_draw(b, seed, p_apply, noise_len, len_b, snr_db=None, snr_lo=0.0, snr_hi=0.0):
    """Clip b's draw for the launch seed `seed` (seed_dev word + by-value seed, mod 2^32): dict(hit, row, offset, snr).  `hit` is the draw's
    part of `applied`; the energies can still turn it off."""
    s = (seed + NOISE_SALT) & M32
    h = [av_pair_hash(s, 4 * b + j) for j in range(4)]
    row = (h[1] * len(noise_len)) >> 32
    offset = (h[2] * int(noise_len[row])) >> 32
    if snr_db is not None:
        snr = as_f32(snr_db[b])
    else:
        lo, hi = as_f32(snr_lo), as_f32(snr_hi)
        snr = as_f32(lo + (hi - lo) * ((h[3] >> 8) * 2.0 ** -24))       # Python floats are doubles and never fuse
    return {"hit": (h[0] >> 8) < threshold(p_apply) and len_b > 0, "row": row, "offset": offset, "snr": snr}


def segment(recording, offset, count):
    """z_i = recording[(offset + i) mod len(recording)], i < count: the segment wraps as often as it has to."""
    nl = len(recording)
    return np.asarray(recording)[(offset + np.arange(count, dtype=np.int64)) % nl]


def energy(x):
    """sum x_i^2 in float64, exactly rounded (math.fsum): the squares of float32 values are exact in double."""
    x = np.asarray(x, dtype=np.float64)
    return math.fsum((x * x).tolist())


def gain64(Es, En, snr):
    """sqrt(Es / (En 10^(snr/10))) in float64; 0.0 where the rule gives up (an energy zero or not finite)."""
    if not (Es > 0.0 and En > 0.0 and math.isfinite(Es) and math.isfinite(En)):
        return 0.0
    return math.sqrt(Es / (En * math.pow(10.0, snr / 10.0)))


def gain32(Es, En, snr):
    with np.errstate(over="ignore"):
        g = float(np.float32(gain64(Es, En, snr)))
    return g if (g > 0.0 and math.isfinite(g)) else 0.0


def mix32(w, z, gain):
    """The kernel's arithmetic: float32 product, rounded, then float32 sum, rounded."""
    w, z = np.asarray(w, dtype=np.float32), np.asarray(z, dtype=np.float32)
    return w + np.float32(gain) * z


def mix64(w, z, gain):
    return np.asarray(w, dtype=np.float64) + float(gain) * np.asarray(z, dtype=np.float64)


def add_noise(wave, lengths, noise, seed, p_apply, snr_db=None, snr_lo=0.0, snr_hi=0.0):
    """wave float32 [B, n], lengths list | None, noise: list of 1-D float32 recordings.  -> (out float32 [B, n] by the kernel's float32 mix,
    info: list of dict(applied, row, offset, snr_db, gain (float32 value), gain64, Es, En, z))."""
    wave = np.asarray(wave, dtype=np.float32)
    B, n = wave.shape
    out, infos = wave.copy(), []
    nlen = [len(r) for r in noise]
    for b in range(B):
        lb = n if lengths is None else max(0, min(n, int(lengths[b])))
        d = noise_draw(b, seed, p_apply, nlen, lb, snr_db, snr_lo, snr_hi)
        info = {"applied": 0, "row": d["row"], "offset": d["offset"], "snr_db": d["snr"], "gain": 0.0, "gain64": 0.0, "Es": 0.0, "En": 0.0, "z": None}
        if d["hit"]:
            z = segment(noise[d["row"]], d["offset"], lb)
            Es, En = energy(wave[b, :lb]), energy(z)
            g = gain32(Es, En, d["snr"])
            info.update(Es=Es, En=En, z=z)
            if g != 0.0:
                info.update(applied=1, gain=g, gain64=gain64(Es, En, d["snr"]))
                out[b, :lb] = mix32(wave[b, :lb], z, g)
        infos.append(info)
    return out, infos


def achieved_snr_db(w, out, len_b):
    """10 log10(Es / sum (out - w)^2) over the clip's own samples, in float64."""
    w, out = np.asarray(w[:len_b], dtype=np.float64), np.asarray(out[:len_b], dtype=np.float64)
    return 10.0 * math.log10(energy(w) / energy(out - w))


# ---------------------------------------------------------------- avllm_spec_augment
def spans(b, seed, valid_b, M, T, n_time, time_width, time_ratio, n_freq, freq_width):
    """[(start, width)] of clip b's masks, time masks first."""
    s = (seed + SPEC_SALT) & M32
    v = T if valid_b is None else max(0, min(T, int(valid_b)))
    out = []
    for j in range(n_time + n_freq):
        h, h2 = av_pair_hash(s, 64 * b + 2 * j), av_pair_hash(s, 64 * b + 2 * j + 1)
        if j < n_time:
            extent, wmax = v, min(int(time_width), int(math.floor(as_f32(time_ratio) * v)))
        else:
            extent, wmax = M, min(int(freq_width), M)
        w = (h * (wmax + 1)) >> 32
        out.append(((h2 * (extent - w + 1)) >> 32, w))
    return out


def masked(sp, n_time, M, T):
    """bool [M, T]: the cells inside any span."""
    m = np.zeros((M, T), dtype=bool)
    for j, (start, w) in enumerate(sp):
        if j < n_time:
            m[:, start:start + w] = True
        else:
            m[start:start + w, :] = True
    return m


def spec_augment(feat, valid, seed, n_time, time_width, time_ratio, n_freq, freq_width, fill):
    """feat float32 [B, M, T] -> (a masked copy, spans int [B, n_time + n_freq, 2]); unmasked cells keep their bits."""
    feat = np.asarray(feat, dtype=np.float32)
    B, M, T = feat.shape
    bits = feat.view(np.uint32).copy()
    fill_bits = np.float32(fill).view(np.uint32)
    all_spans = []
    for b in range(B):
        sp = spans(b, seed, None if valid is None else valid[b], M, T, n_time, time_width, time_ratio, n_freq, freq_width)
        bits[b][masked(sp, n_time, M, T)] = fill_bits
        all_spans.append(sp)
    return bits.view(np.float32), np.asarray(all_spans, dtype=np.int64).reshape(B, n_time + n_freq, 2)


def augment_seed(base, step, rank):
    """The trainer's seed for the batch of optimizer step `step` (0-based count of steps taken before it) on `rank`."""
    return (base + 1000003 * step + 7919 * rank) & M32
