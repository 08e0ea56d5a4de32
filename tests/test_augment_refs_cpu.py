"""CPU: the restatements of tests/refs64_augment.py and the bars of tests/bars_augment.py, before any kernel is compared with them: the draw
against a second formulation (numpy uint64 vectors instead of Python integers), its determinism and frequencies, the float32 emulation of
the mix under every bar, and planted faults, each of which has to land over a bar."""
import math

import numpy as np
import pytest

import bars_augment as BA
import refs64_augment as RA
from refs64_modality import threshold

U = np.uint64


def hash32_v(x):
    x = x & U(0xFFFFFFFF)
    x = x ^ (x >> U(16))
    x = (x * U(0x7FEB352D)) & U(0xFFFFFFFF)
    x = x ^ (x >> U(15))
    x = (x * U(0x846CA68B)) & U(0xFFFFFFFF)
    return x ^ (x >> U(16))


def pair_hash_v(seed, pair):
    """av_pair_hash for pairs below 2^32, vectorised."""
    return hash32_v(pair.astype(U) ^ hash32_v(np.asarray([seed], dtype=U)))


@pytest.mark.parametrize("seed", [0, 12345, 0xDEADBEEF, 0xFFFFFFFF])
def test_draw_equals_second_formulation(seed):
    B, p = 257, 0.37
    nlen = [1, 7, 4099, 16000, 480001]
    s = (seed + RA.NOISE_SALT) & 0xFFFFFFFF
    b = np.arange(B, dtype=U)
    h = [pair_hash_v(s, U(4) * b + U(j)) for j in range(4)]
    hit = (h[0] >> U(8)) < U(threshold(p))
    row = (h[1] * U(len(nlen))) >> U(32)
    off = (h[2] * np.asarray(nlen, dtype=U)[row.astype(np.int64)]) >> U(32)
    lo, hi = np.float64(np.float32(-7.5)), np.float64(np.float32(22.25))
    snr = (lo + (hi - lo) * ((h[3] >> U(8)).astype(np.float64) * 2.0 ** -24)).astype(np.float32)
    for i in range(B):
        d = RA.noise_draw(i, seed, p, nlen, 5, None, -7.5, 22.25)
        assert (d["hit"], d["row"], d["offset"]) == (bool(hit[i]), int(row[i]), int(off[i])), i
        assert np.float32(d["snr"]).view(np.uint32) == snr[i].view(np.uint32), i
        assert 0 <= d["offset"] < nlen[d["row"]] and -7.5 <= d["snr"] <= 22.25
        assert RA.noise_draw(i, seed, p, nlen, 0)["hit"] is False                       # an empty clip is never mixed
        assert RA.noise_draw(i, seed, p, nlen, 5, snr_db=[3.0] * B)["snr"] == 3.0       # a given SNR is taken, the rest of the draw unchanged
    # spans: the same hashes, formed the second way
    s2 = (seed + RA.SPEC_SALT) & 0xFFFFFFFF
    for bb in (0, 3, 200):
        sp = RA.spans(bb, seed, 900, 80, 3000, 2, 100, 0.2, 2, 27)
        for j, (start, w) in enumerate(sp):
            hh = pair_hash_v(s2, np.asarray([64 * bb + 2 * j, 64 * bb + 2 * j + 1], dtype=U))
            extent, wmax = (900, min(100, 180)) if j < 2 else (80, 27)
            w2 = int((hh[0] * U(wmax + 1)) >> U(32))
            assert (start, w) == (int((hh[1] * U(extent - w2 + 1)) >> U(32)), w2)
            assert 0 <= w <= wmax and 0 <= start and start + w <= extent


def test_draw_is_deterministic_and_has_the_right_share():
    N, p, nlen = 4096, 0.3, [100, 50]
    a = [RA.noise_draw(b, 777, p, nlen, 9) for b in range(N)]
    assert a == [RA.noise_draw(b, 777, p, nlen, 9) for b in range(N)]
    share = sum(d["hit"] for d in a) / N
    assert abs(share - p) <= 4 * math.sqrt(p * (1 - p) / N), share
    rows = sum(d["row"] for d in a) / N
    assert abs(rows - 0.5) <= 4 * math.sqrt(0.25 / N), rows
    assert all(RA.noise_draw(b, 777, 1.0, nlen, 9)["hit"] for b in range(64)) and not any(RA.noise_draw(b, 777, 0.0, nlen, 9)["hit"] for b in range(64))
    # row and offset do not depend on the SNR
    for b in range(16):
        x, y = RA.noise_draw(b, 5, 1.0, nlen, 9, snr_db=[-10.0] * 16), RA.noise_draw(b, 5, 1.0, nlen, 9, snr_db=[30.0] * 16)
        assert (x["row"], x["offset"]) == (y["row"], y["offset"])


# ---------------------------------------------------------------- the emulation under the bars, the faults over them
def case(seed=3, B=6, n=9000, pad=(0, 1, 500, 4097, 0, 33)):
    g = np.random.default_rng(seed)
    wave = (0.1 * g.standard_normal((B, n))).astype(np.float32)
    lengths = [n - pad[b % len(pad)] for b in range(B)]
    for b in range(B):
        wave[b, lengths[b]:] = 0.25 + b                       # loud padding: a rule that lets it into Es shows
    noise = [(0.3 * g.standard_normal(m)).astype(np.float32) for m in (7, 4099, 2000, 12001)]
    noise[1][:2000] *= 8.0                                    # a recording whose energy is not that of any one segment
    snr = [-10.0, -5.0, 0.0, 5.0, 10.0, 30.0]
    return wave, lengths, noise, snr


def violations(wave, lengths, noise, snr, seed, out, gains, rows_offsets=None):
    """Which bars a candidate (out [B, n], gains [B]) is over, against the float64 rule."""
    _, infos = RA.add_noise(wave, lengths, noise, seed, 1.0, snr_db=snr)
    bad = set()
    for b, info in enumerate(infos):
        lb, g, z = lengths[b], info["gain64"], info["z"]
        if rows_offsets is not None and rows_offsets[b] != (info["row"], info["offset"]):
            bad.add("draw")
        if abs(gains[b] - g) > BA.gain_bar(g, lb):
            bad.add("gain")
        if np.any(np.abs(out[b, :lb].astype(np.float64) - RA.mix64(wave[b, :lb], z, g)) > BA.mix_bar(wave[b, :lb], z, g, lb)):
            bad.add("mix")
        if abs(RA.achieved_snr_db(wave[b], out[b], lb) - snr[b]) > BA.snr_bar_db(wave[b, :lb], z, g, lb):
            bad.add("snr")
        if not np.array_equal(BA.bits(out[b, lb:]), BA.bits(wave[b, lb:])):
            bad.add("copy")
    return bad


def candidate(wave, lengths, noise, snr, seed, energy_of_noise=None, gain_of=None, seg=None, offset_of=None, signal_upto=None, apply_gain=None):
    """The rule with one step replaced."""
    out, gains, ro = wave.copy(), [], []
    nlen = [len(r) for r in noise]
    for b in range(wave.shape[0]):
        lb = lengths[b]
        d = RA.noise_draw(b, seed, 1.0, nlen, lb, snr_db=snr)
        off = d["offset"] if offset_of is None else offset_of(b, d, noise)
        z = (seg or RA.segment)(noise[d["row"]], off, lb)
        Es = RA.energy(wave[b, :(lb if signal_upto is None else signal_upto(b))])
        En = RA.energy(z) if energy_of_noise is None else energy_of_noise(noise[d["row"]], lb)
        g = (gain_of or RA.gain32)(Es, En, d["snr"])
        out[b, :lb] = (apply_gain or RA.mix32)(wave[b, :lb], z, g)
        gains.append(g); ro.append((d["row"], off))
    return out, gains, ro


def test_emulation_is_under_every_bar():
    wave, lengths, noise, snr = case()
    for seed in (3, 99):
        out, infos = RA.add_noise(wave, lengths, noise, seed, 1.0, snr_db=snr)
        assert all(i["applied"] for i in infos)
        assert violations(wave, lengths, noise, snr, seed, out, [i["gain"] for i in infos], [(i["row"], i["offset"]) for i in infos]) == set()
        out2, gains, ro = candidate(wave, lengths, noise, snr, seed)
        assert np.array_equal(BA.bits(out), BA.bits(out2)) and violations(wave, lengths, noise, snr, seed, out2, gains, ro) == set()
    # a clip or a recording of zeros: unchanged, applied = 0
    z = np.zeros((2, 50), np.float32)
    out, infos = RA.add_noise(z, None, noise, 1, 1.0, snr_db=[0.0, 0.0])
    assert not out.any() and [i["applied"] for i in infos] == [0, 0]
    out, infos = RA.add_noise(wave[:2, :50], None, [np.zeros(9, np.float32)], 1, 1.0, snr_db=[0.0, 0.0])
    assert np.array_equal(out, wave[:2, :50]) and [i["applied"] for i in infos] == [0, 0] and [i["gain"] for i in infos] == [0.0, 0.0]


def late_wrap(recording, offset, count):
    padded = np.concatenate([np.asarray(recording), np.zeros(1, np.float32)])       # the padded image's next cell
    return padded[(offset + np.arange(count)) % (len(recording) + 1)]


FAULTS = {
    "noise energy of the whole recording": dict(energy_of_noise=lambda rec, lb: RA.energy(rec) * lb / len(rec)),
    "gain applied squared": dict(apply_gain=lambda w, z, g: RA.mix32(w, z, np.float32(g) * np.float32(g))),
    "SNR sign flipped": dict(gain_of=lambda Es, En, snr: RA.gain32(Es, En, -snr)),
    "wrap one sample late": dict(seg=late_wrap),
    "offset modulo the padded width": dict(offset_of=lambda b, d, noise: (RA.av_pair_hash((3 + RA.NOISE_SALT) & 0xFFFFFFFF, 4 * b + 2) * 12004) >> 32),
    "padding included in Es": dict(signal_upto=lambda b: 9000),
}


@pytest.mark.parametrize("name", sorted(FAULTS))
def test_planted_noise_fault_is_over_a_bar(name):
    wave, lengths, noise, snr = case()
    kw = dict(FAULTS[name])
    if name == "offset modulo the padded width":                # the faulty offset can leave the recording: read it modulo, as the image would allow
        kw["seg"] = lambda rec, off, count: np.concatenate([rec, np.zeros(12004 - len(rec), np.float32)])[(off + np.arange(count)) % 12004]
    out, gains, ro = candidate(wave, lengths, noise, snr, 3, **kw)
    assert violations(wave, lengths, noise, snr, 3, out, gains, ro), name


def test_planted_span_faults_are_seen():
    args = dict(M=80, T=3000, n_time=2, time_width=100, time_ratio=1.0, n_freq=2, freq_width=27)
    s = (11 + RA.SPEC_SALT) & 0xFFFFFFFF
    past_valid = narrow = 0
    for b in range(64):
        valid = 150 + b
        sp = RA.spans(b, 11, valid, **args)
        assert all(st + w <= valid for st, w in sp[:2]) and all(st + w <= 80 for st, w in sp[2:])
        m = RA.masked(sp, 2, 80, 3000)
        assert not m[:, valid:][~m[:, 0], :].any()              # beyond valid only whole frequency rows are masked
        for j in range(4):
            h, h2 = RA.av_pair_hash(s, 64 * b + 2 * j), RA.av_pair_hash(s, 64 * b + 2 * j + 1)
            wmax = 100 if j < 2 else 27
            w = (h * (wmax + 1)) >> 32
            if j < 2:
                fault = ((h2 * (3000 - w + 1)) >> 32, w)        # a time span placed in all T frames
                past_valid += fault != sp[j] and fault[0] + fault[1] > valid
            narrow += ((h * wmax) >> 32) != sp[j][1]            # a width from [0, W)
    assert past_valid > 32 and narrow > 0
    # widths reach both ends of [0, W] over enough draws
    ws = [RA.spans(b, 5, None, 8, 40, 1, 3, 1.0, 0, 0)[0][1] for b in range(256)]
    assert set(ws) == {0, 1, 2, 3}
    # valid = 0: zero-width time spans; the ratio cap
    assert RA.spans(0, 5, 0, 8, 40, 2, 3, 1.0, 0, 0) == [(0, 0), (0, 0)]
    assert all(w <= 5 for _, w in RA.spans(1, 5, 27, 8, 40, 4, 30, 0.2, 0, 0))


def test_spec_augment_keeps_unmasked_bits():
    g = np.random.default_rng(0)
    feat = g.standard_normal((3, 8, 40)).astype(np.float32)
    feat[0, 0, 0], feat[1, 3, 5], feat[2, 7, 39] = np.nan, -0.0, np.inf
    out, sp = RA.spec_augment(feat, [40, 17, 0], 9, 2, 6, 1.0, 1, 3, 0.5)
    for b in range(3):
        m = RA.masked([tuple(x) for x in sp[b]], 2, 8, 40)
        assert np.all(out[b][m] == np.float32(0.5)) and np.array_equal(BA.bits(out[b][~m]), BA.bits(feat[b][~m]))
    assert RA.augment_seed(5, 0, 0) == 5 and RA.augment_seed(5, 3, 0) != RA.augment_seed(5, 3, 1) and RA.augment_seed(2 ** 32 - 1, 1, 1) == (1000003 + 7919 - 1)
