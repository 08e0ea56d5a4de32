"""The acoustic augmentation kernels (csrc/augment.hip) through the C ABI against tests/refs64_augment.py under the bars of
tests/bars_augment.py.  Every output lies inside a sentinel-guarded buffer, rows with a stride wider than the row, and what the rule says is
copied or left alone is compared by bits."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars_augment as BA  # noqa: E402
import refs64_augment as RA  # noqa: E402
from avllm import lib as L  # noqa: E402

GUARD = 64                       # floats in front of and behind every buffer (keeps the payload 256-byte aligned)
SENT = 0x7FC0BEEF                # a NaN with a payload: any arithmetic on it, or any write over it, shows
NAN_PAD = np.uint32(0x7FC01234).view(np.float32)


def chunk():
    return int(L.load().avllm_wave_add_noise_chunk())


class Guarded:
    """A float32 / int32 device buffer of `rows` rows of `width` cells at row stride `ld`, between two guards, everything outside the rows'
    cells holding SENT."""

    def __init__(self, dev, rows, width, ld=None, dtype=torch.float32):
        self.rows, self.width, self.ld = rows, width, ld or width
        self.buf = torch.full((2 * GUARD + rows * self.ld,), SENT, dtype=torch.int32, device=dev)
        self.dtype = dtype

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def view(self):
        return self.buf[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width]

    def put(self, a):
        self.view().copy_(torch.from_numpy(np.ascontiguousarray(a)).view(torch.int32).to(self.buf.device))
        return self

    def get(self):
        """The payload as numpy (dtype as declared); asserts that guards and row gaps still hold the sentinel."""
        host = self.buf.cpu().numpy()
        body = host[GUARD:GUARD + self.rows * self.ld].reshape(self.rows, self.ld)
        assert (host[:GUARD] == SENT).all() and (host[GUARD + self.rows * self.ld:] == SENT).all(), "a guard was written"
        assert (body[:, self.width:] == SENT).all(), "the gap between two rows was written"
        out = np.ascontiguousarray(body[:, :self.width])
        return out.view(np.float32) if self.dtype == torch.float32 else out


def bank(dev, noise):
    width = (max(len(r) for r in noise) + 3) // 4 * 4
    img = np.zeros((len(noise), width), np.float32)
    for i, r in enumerate(noise):
        img[i, :len(r)] = r
    return torch.from_numpy(img).to(dev), torch.tensor([len(r) for r in noise], dtype=torch.int32, device=dev), width


def add_noise(dev, wave, lengths, noise, seed, p, snr_db=None, lo=0.0, hi=0.0, extra=0, seed_dev=None, in_place=False, check=True):
    """One avllm_wave_add_noise call.  -> (out [B, n] float32, info dict of lists).  extra: cells added to both row strides."""
    lib = L.load()
    B, n = wave.shape
    src = Guarded(dev, B, n, n + extra).put(wave)
    dst = src if in_place else Guarded(dev, B, n, n + extra + (0 if extra else 4))
    info = Guarded(dev, B, 5, dtype=torch.int32)
    img, nlen, _ = bank(dev, noise)
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    snr = None if snr_db is None else torch.tensor(snr_db, dtype=torch.float32, device=dev)
    need = lib.avllm_wave_add_noise_workspace_bytes(B, n)
    ws = Guarded(dev, 1, need // 4)
    rc = lib.avllm_wave_add_noise(src.ptr, src.ld, L.ptr(lens), B, n, L.ptr(img), img.stride(0), L.ptr(nlen), len(noise), L.ptr(snr), lo, hi, p,
                                  seed & 0xFFFFFFFF, L.ptr(seed_dev), dst.ptr, dst.ld, info.ptr, ws.ptr, need, L.stream_ptr())
    L.check(rc)
    torch.cuda.synchronize()
    ws.get()
    if not in_place:
        assert np.array_equal(BA.bits(src.get()), BA.bits(wave)), "the input was written"
    raw = info.get()
    f = raw.view(np.float32)
    got = {"applied": raw[:, 0].tolist(), "row": raw[:, 1].tolist(), "offset": raw[:, 2].tolist(), "snr_db": f[:, 3].copy(), "gain": f[:, 4].copy()}
    out = dst.get()
    if check:
        compare(wave, lengths, noise, seed, p, snr_db, lo, hi, out, got)
    return out, got


def compare(wave, lengths, noise, seed, p, snr_db, lo, hi, out, got, seed_total=None):
    """The kernel's outputs against the restatement: integers and the SNR by bits, the gain and the mix under their bars, the achieved SNR
    under its bar, copies by bits; and the mix equals the float32 emulation run with the kernel's own gain, bit for bit."""
    B, n = wave.shape
    _, infos = RA.add_noise(wave, lengths, noise, seed if seed_total is None else seed_total, p, snr_db, lo, hi)
    for b, info in enumerate(infos):
        lb = n if lengths is None else max(0, min(n, lengths[b]))
        what = f"clip {b} len {lb}"
        assert (got["applied"][b], got["row"][b], got["offset"][b]) == (info["applied"], info["row"], info["offset"]), what
        assert got["snr_db"][b].view(np.uint32) == np.float32(info["snr_db"]).view(np.uint32), what
        assert np.array_equal(BA.bits(out[b, lb:]), BA.bits(wave[b, lb:])), what + ": padding not copied bit for bit"
        if not info["applied"]:
            assert got["gain"][b] == 0.0 and np.array_equal(BA.bits(out[b]), BA.bits(wave[b])), what + ": an unmixed clip changed"
            continue
        g, z, w = info["gain64"], info["z"], wave[b, :lb]
        assert np.isfinite(got["gain"][b]) and abs(float(got["gain"][b]) - g) <= BA.gain_bar(g, lb), (what, float(got["gain"][b]), g)
        err = np.abs(out[b, :lb].astype(np.float64) - RA.mix64(w, z, g))
        bar = BA.mix_bar(w, z, g, lb)
        assert np.all(err <= bar), (what, float((err / bar).max()))
        assert np.array_equal(BA.bits(out[b, :lb]), BA.bits(RA.mix32(w, z, got["gain"][b]))), what + ": not the float32 product-then-sum"
        got_snr = RA.achieved_snr_db(wave[b], out[b], lb)
        assert abs(got_snr - info["snr_db"]) <= BA.snr_bar_db(w, z, g, lb), (what, got_snr, info["snr_db"])


def clips(B, n, seed=0, nan_pad=None):
    g = np.random.default_rng(seed)
    w = (0.1 * g.standard_normal((B, n))).astype(np.float32)
    if nan_pad is not None:
        for b, lb in enumerate(nan_pad):
            w[b, lb:] = NAN_PAD
    return w


def recordings(lengths, seed=1):
    g = np.random.default_rng(seed)
    return [(0.3 * g.standard_normal(m)).astype(np.float32) for m in lengths]


@pytest.mark.parametrize("given", [True, False])
@pytest.mark.parametrize("extra", [0, 1])
def test_mix_lengths_strides_and_nan_padding(dev, extra, given):
    C = chunk()
    n = 4 * C + 8
    lengths = [0, 1, C - 1, C, C + 1, 3 * C + 5, n]
    wave = clips(len(lengths), n, 0, nan_pad=lengths)
    snr = [-10.0, -5.0, 0.0, 7.5, 10.0, 20.0, 30.0] if given else None
    out, got = add_noise(dev, wave, lengths, recordings([5000, 20001]), 17, 1.0, snr, -10.0, 30.0, extra=extra)
    assert got["applied"] == [0, 1, 1, 1, 1, 1, 1] and np.isfinite(got["gain"]).all()
    assert np.isfinite(out[1, :1]).all() and np.isfinite(out[5, :3 * C + 5]).all()
    for B in (3, 8):                                                  # other batch sizes, lengths None
        add_noise(dev, clips(B, C + 3, B), None, recordings([5000, 20001]), 17, 1.0, None, -10.0, 30.0, extra=extra)


def test_mix_thirty_seconds(dev):
    n = 480000
    lengths = [n, n - 3]
    add_noise(dev, clips(2, n, 5, nan_pad=lengths), lengths, recordings([160000, 777]), 3, 1.0, [5.0, -10.0])


def find_seed(nlen, B, want):
    for seed in range(4096):
        ds = [RA.noise_draw(b, seed, 1.0, nlen, 1) for b in range(B)]
        if want(ds):
            return seed
    raise AssertionError("no seed with the wanted draws")


@pytest.mark.parametrize("extra", [0, 1])
def test_noise_lengths_offsets_and_wraps(dev, extra):
    C = chunk()
    nlen, n, B = [1, 7, C + 3, 3 * C], 2 * C + 10, 8
    seed = find_seed(nlen, B, lambda ds: {d["row"] for d in ds} == {0, 1, 2, 3}
                     and any(d["offset"] == 0 and nlen[d["row"]] > 1 for d in ds)
                     and any(d["offset"] == nlen[d["row"]] - 1 and nlen[d["row"]] > 1 for d in ds))
    out, got = add_noise(dev, clips(B, n, 2), None, recordings(nlen, 4), seed, 1.0, None, 0.0, 10.0, extra=extra)
    assert set(got["row"]) == {0, 1, 2, 3}                            # rows 0, 1 wrap hundreds of times, row 2 once or twice, row 3 is longer than the clip
    assert all(got["applied"])


def test_probabilities(dev):
    C = chunk()
    wave, noise = clips(4, C + 9, 7), recordings([300, 5000])
    out, got = add_noise(dev, wave, None, noise, 5, 0.0, None, 0.0, 10.0)
    assert got["applied"] == [0] * 4 and np.array_equal(BA.bits(out), BA.bits(wave))
    out, got = add_noise(dev, wave, [C, 9, 0, C + 9], noise, 5, 0.0, None, 0.0, 10.0, in_place=True, extra=1)
    assert got["applied"] == [0] * 4 and np.array_equal(BA.bits(out), BA.bits(wave))
    out, got = add_noise(dev, wave, None, noise, 5, 1.0, None, 0.0, 10.0, in_place=True)
    assert got["applied"] == [1] * 4
    out, got = add_noise(dev, clips(64, 260, 8), None, noise, 5, 0.5, None, -10.0, 30.0)
    assert 16 <= sum(got["applied"]) <= 48                          # the exact set is compared with the restatement inside add_noise


def test_silence_is_left_alone(dev):
    wave = clips(3, 700, 9)
    wave[1] = 0.0
    out, got = add_noise(dev, wave, None, recordings([300]), 5, 1.0, [0.0] * 3)
    assert got["applied"] == [1, 0, 1] and not out[1].any()
    out, got = add_noise(dev, wave, None, [np.zeros(300, np.float32)], 5, 1.0, [0.0] * 3)
    assert got["applied"] == [0, 0, 0] and np.array_equal(BA.bits(out), BA.bits(wave))


def test_seed_word_repeat_and_snr_sweep(dev):
    wave, noise = clips(5, 3000, 10), recordings([300, 5000, 41])
    base, got0 = add_noise(dev, wave, None, noise, 1234, 1.0, None, -10.0, 30.0)
    # the device word and the by-value seed add up mod 2^32
    word = torch.tensor([-100], dtype=torch.int32, device=dev)        # 2^32 - 100
    out, got = add_noise(dev, wave, None, noise, 1334, 1.0, None, -10.0, 30.0, seed_dev=word, check=False)
    compare(wave, None, noise, None, 1.0, None, -10.0, 30.0, out, got, seed_total=1234)
    assert np.array_equal(BA.bits(out), BA.bits(base))
    # two launches: equal bits, info included
    again, got1 = add_noise(dev, wave, None, noise, 1234, 1.0, None, -10.0, 30.0, check=False)
    assert np.array_equal(BA.bits(again), BA.bits(base)) and np.array_equal(BA.bits(got1["gain"]), BA.bits(got0["gain"]))
    # a sweep over the SNR at one seed keeps row and offset; the gain follows 10^(-snr/20)
    gains = []
    for snr in (-10.0, 0.0, 10.0, 30.0):
        _, g = add_noise(dev, wave, None, noise, 1234, 1.0, [snr] * 5)
        assert (g["row"], g["offset"]) == (got0["row"], got0["offset"])
        gains.append(g["gain"].astype(np.float64))
    assert np.allclose(gains[0] / gains[1], 10 ** 0.5, rtol=1e-6) and np.allclose(gains[1] / gains[3], 10 ** 1.5, rtol=1e-6)


# ---------------------------------------------------------------- SpecAugment
def spec(dev, feat, valid, seed, nt, tw, ratio, nf, fw, fill, seed_dev=None):
    B, M, T = feat.shape
    buf = Guarded(dev, 1, B * M * T).put(feat.reshape(1, -1))
    spans = Guarded(dev, 1, B * (nt + nf) * 2, dtype=torch.int32)
    v = None if valid is None else torch.tensor(valid, dtype=torch.int32, device=dev)
    L.check(L.load().avllm_spec_augment(buf.ptr, B, M, T, L.ptr(v), nt, tw, ratio, nf, fw, fill, seed & 0xFFFFFFFF, L.ptr(seed_dev), spans.ptr,
                                        L.stream_ptr()))
    torch.cuda.synchronize()
    return buf.get().reshape(B, M, T), spans.get().reshape(B, nt + nf, 2)


def sprinkled(B, M, T, seed):
    g = np.random.default_rng(seed)
    f = g.standard_normal((B, M, T)).astype(np.float32)
    f.reshape(-1)[g.integers(0, f.size, size=max(8, f.size // 97))] = NAN_PAD
    f.reshape(-1)[g.integers(0, f.size, size=8)] = -0.0
    return f


@pytest.mark.parametrize("B,M,T,valid", [(4, 80, 3000, [0, 1, 60, 3000]), (4, 128, 3000, [2999, 7, 0, 1500]), (5, 6, 37, [0, 1, 5, 37, 20]),
                                         (3, 80, 3000, None)])
def test_spec_augment_is_the_restatement(dev, B, M, T, valid):
    feat = sprinkled(B, M, T, M + T)
    for seed, (nt, tw, ratio, nf, fw, fill) in enumerate([(2, 100, 1.0, 2, 27, 0.0), (10, 50, 0.05, 0, 0, -1.5), (0, 0, 1.0, 3, 200, 0.25),
                                                          (16, 3000, 1.0, 16, 4, 0.0)]):
        want, want_spans = RA.spec_augment(feat, valid, 40 + seed, nt, tw, ratio, nf, fw, fill)
        got, got_spans = spec(dev, feat, valid, 40 + seed, nt, tw, ratio, nf, fw, fill)
        assert np.array_equal(got_spans, want_spans), (seed, got_spans.tolist(), want_spans.tolist())
        assert np.array_equal(BA.bits(got), BA.bits(want)), seed
        for b in range(B):                                            # stated once more without the restated fill: masked = fill, the rest = input bits
            m = RA.masked([tuple(x) for x in want_spans[b]], nt, M, T)
            assert np.all(BA.bits(got[b][m]) == BA.bits(np.float32(fill))) and np.array_equal(BA.bits(got[b][~m]), BA.bits(feat[b][~m]))
            if valid is not None:
                assert all(st + w <= valid[b] for st, w in want_spans[b][:nt])
    word = torch.tensor([-3], dtype=torch.int32, device=dev)
    got, got_spans = spec(dev, feat, valid, 43, 2, 100, 1.0, 2, 27, 0.0, seed_dev=word)
    want, want_spans = RA.spec_augment(feat, valid, 40, 2, 100, 1.0, 2, 27, 0.0)
    assert np.array_equal(got_spans, want_spans) and np.array_equal(BA.bits(got), BA.bits(want))


def test_spec_augment_without_masks_launches_nothing(dev):
    # NULL tensors: a launch would fault, the entry returns before it looks at them
    L.check(L.load().avllm_spec_augment(None, 4, 80, 3000, None, 0, 100, 1.0, 0, 27, 0.0, 1, None, None, L.stream_ptr()))
    torch.cuda.synchronize()


def test_argument_errors_name_the_offender(dev):
    lib = L.load()
    wave = torch.zeros(2, 64, device=dev)
    out, info = torch.zeros(2, 64, device=dev), torch.zeros(2, 5, dtype=torch.int32, device=dev)
    img, nlen = torch.ones(1, 8, device=dev), torch.tensor([8], dtype=torch.int32, device=dev)
    need = lib.avllm_wave_add_noise_workspace_bytes(2, 64)
    assert need == 2 * ((64 + chunk() - 1) // chunk()) * 16
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=dev)

    def call(p=1.0, lo=0.0, hi=10.0, Nn=1, ws_bytes=need, noise=img, ld_out=64, dst=out):
        return lib.avllm_wave_add_noise(L.ptr(wave), 64, None, 2, 64, L.ptr(noise), 8, L.ptr(nlen), Nn, None, lo, hi, p, 0, None, L.ptr(dst), ld_out,
                                        L.ptr(info), L.ptr(ws), ws_bytes, L.stream_ptr())

    L.check(call())
    for kw, msg in ((dict(p=1.5), "p_apply=1.5"), (dict(p=-0.1), "p_apply=-0.1"), (dict(lo=5.0, hi=1.0), "snr_lo=5 > snr_hi=1"), (dict(Nn=0), "Nn=0"),
                    (dict(ws_bytes=need - 1), "workspace too small"), (dict(noise=None), "noise bank"), (dict(ld_out=63), "ld_out=63"),
                    (dict(dst=wave, ld_out=80), "out aliases wave")):
        with pytest.raises(ValueError, match=msg):
            L.check(call(**kw))
    feat, spans = torch.zeros(2, 8, 16, device=dev), torch.zeros(2, 33, 2, dtype=torch.int32, device=dev)

    def mask(nt=1, tw=4, ratio=1.0, nf=1, fw=2, f=feat):
        return lib.avllm_spec_augment(L.ptr(f), 2, 8, 16, None, nt, tw, ratio, nf, fw, 0.0, 0, None, L.ptr(spans), L.stream_ptr())

    L.check(mask())
    for kw, msg in ((dict(nt=20, nf=13), r"n_time=20 \+ n_freq=13"), (dict(nt=-1), "n_time=-1"), (dict(ratio=1.5), "max_time_ratio=1.5"),
                    (dict(tw=-2), "max_time_width=-2"), (dict(f=None), "feat NULL")):
        with pytest.raises(ValueError, match=msg):
            L.check(mask(**kw))
    torch.cuda.synchronize()
