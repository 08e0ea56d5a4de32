"""The kernels of the fp8 KV cache (csrc/kv_fp8.hip, and its reader in csrc/attention_decode.hip) one by one: the prefill append and the token step's rotate-and-append against the MX rule
of oracle/mxfp8.py bit for bit (and, where a rotation by real angles precedes the rule, against float64 within the rule's own half ulp), the
single-token attention over the image against refs64_attention on the dequantised values with test_attention_pin_gpu.py::test_decode's bars, and
the beam gather byte for byte.  Images are read and built only through ops.kv8_unpack / ops.kv8_pack."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64_attention as A  # noqa: E402
import refs64_kv8 as R8  # noqa: E402
from avllm import ops  # noqa: E402
from oracle import mxfp8  # noqa: E402
from test_attention_pin_gpu import check  # noqa: E402

BF = torch.bfloat16
SENT = 0xA5                      # every byte of a cache before a kernel writes into it
GEOS = [(128, 64), (128, 128), (512, 64), (512, 128)]            # (dkv, head_dim)


def rows_bf16(n, width, seed):
    """[n, width] bf16 on the CPU: N(0, 1) rows with, in row 0, an all-zero MX block (exponent byte 0) and a block whose largest element, 1.9375 =
    496 / 256, lies above 448 / 256 of its power of two and so saturates."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, width, generator=g)
    x[0, :32] = 0.0
    x[0, 32:64] = x[0, 32:64].clamp(-0.9, 0.9)
    x[0, 40] = 1.9375
    return x.to(BF)


def mx_bytes(x):
    """oracle.mxfp8.quantize as the image stores it: (codes uint8, exponent bytes uint8)."""
    q, e = mxfp8.quantize(x.float())
    return q, (e + 127).to(torch.uint8)


def sentinel_caches(B, Tmax, dkv):
    kc, vc = ops.kv8_alloc(B, Tmax, dkv=dkv), ops.kv8_alloc(B, Tmax, dkv=dkv)
    kc.fill_(SENT); vc.fill_(SENT)
    return kc, vc


def check_rows(cache, pos, want_q, want_e, what):
    """Positions `pos` (a slice) of the image hold exactly want_q / want_e, every other byte is the sentinel."""
    q, e = (t.cpu() for t in ops.kv8_unpack(cache))
    assert torch.equal(q[:, pos], want_q), f"{what}: codes differ in {int((q[:, pos] != want_q).sum())} places"
    assert torch.equal(e[:, pos], want_e), f"{what}: exponents differ in {int((e[:, pos] != want_e).sum())} places"
    keep = torch.ones(q.shape[1], dtype=torch.bool)
    keep[pos] = False
    assert bool((q[:, keep] == SENT).all()) and bool((e[:, keep] == SENT).all()), f"{what}: wrote outside its rows"


@pytest.mark.parametrize("dkv,hd", GEOS)
def test_prefill_append_is_the_mx_rule(dev, dkv, hd):
    B, T, pos0, Tmax = 2, 5, 3, 11
    d = 2 * dkv
    qkv = torch.cat([rows_bf16(B * T, d, 1), rows_bf16(B * T, dkv, 2), rows_bf16(B * T, dkv, 3)], 1)
    k, v = qkv[:, d:d + dkv], qkv[:, d + dkv:]
    kc, vc = sentinel_caches(B, Tmax, dkv)
    g = qkv.to(dev)
    ops.kv8_append(g[:, d:d + dkv], g[:, d + dkv:], kc, vc, T, pos0)
    for name, cache, x in (("k", kc, k), ("v", vc, v)):
        wq, we = mx_bytes(x)
        assert int(we.min()) == 0 and bool((wq.view(torch.float8_e4m3fn).float().abs() == 448).any()), "the zero and the saturating block are in the input"
        check_rows(cache, slice(pos0, pos0 + T), wq.view(B, T, dkv), we.view(B, T, dkv // 32), f"kv8_append {name} dkv={dkv}")


def rotate64(x, cos, sin, heads, hd):
    """HF's rotate_half pairing (i, i + hd/2) on [rows, heads * hd], float64; cos, sin [hd/2]."""
    t = x.double().view(x.shape[0], heads, 2, hd // 2)
    a, b = t[:, :, 0], t[:, :, 1]
    return torch.stack([a * cos - b * sin, b * cos + a * sin], 2).reshape(x.shape[0], heads * hd)


@pytest.mark.parametrize("dkv,hd", GEOS)
def test_token_step_append_exact_tables(dev, dkv, hd):
    """Rotations that are exact in any arithmetic (cos = 1, sin = 0; cos = 0, sin = +-1, mixed over the frequencies): the rotated k is a bf16 row,
    so codes and exponents are the MX rule of it bit for bit, q is that rotation bit for bit, v is the rule of the projected row.  Position from
    the host and from device memory; rotate=False stores k as it is and leaves q alone."""
    B, Tmax, pos = 3, 9, 5
    Hkv = dkv // hd
    H = 2 * Hkv
    d = H * hd
    qkv = torch.cat([rows_bf16(B, d, 4), rows_bf16(B, dkv, 5), rows_bf16(B, dkv, 6)], 1)
    i = torch.arange(hd // 2)
    cos = torch.where(i % 3 == 0, 1.0, 0.0).double()
    sin = torch.where(i % 3 == 1, 1.0, torch.where(i % 3 == 2, -1.0, 0.0)).double()
    tab = torch.stack([cos, sin], -1).float().contiguous().to(dev)
    q_want = rotate64(qkv[:, :d], cos, sin, H, hd).to(BF)
    k_want = rotate64(qkv[:, d:d + dkv], cos, sin, Hkv, hd).to(BF)
    assert torch.equal(k_want.double(), rotate64(qkv[:, d:d + dkv], cos, sin, Hkv, hd))          # exact: the rotated row IS a bf16 row
    for use_dev in (False, True):
        kc, vc = sentinel_caches(B, Tmax, dkv)
        g = qkv.to(dev)
        pd = torch.tensor([3], device=dev, dtype=torch.int32) if use_dev else None
        ops.kv8_rope_append_(g, H, Hkv, hd, tab, kc, vc, pos=pos - (3 if use_dev else 0), pos_dev=pd)
        assert torch.equal(g[:, :d].cpu(), q_want) and torch.equal(g[:, d:].cpu(), qkv[:, d:]), "q rotated in place, k and v columns untouched"
        for name, cache, x in (("k", kc, k_want), ("v", vc, qkv[:, d + dkv:])):
            wq, we = mx_bytes(x)
            check_rows(cache, slice(pos, pos + 1), wq.view(B, 1, dkv), we.view(B, 1, dkv // 32), f"kv8_rope_append {name} dkv={dkv} hd={hd} dev={use_dev}")
    kc, vc = sentinel_caches(B, Tmax, dkv)
    g = qkv.to(dev)
    ops.kv8_rope_append_(g, H, Hkv, hd, None, kc, vc, pos=pos, rotate=False)
    assert torch.equal(g.cpu(), qkv)
    wq, we = mx_bytes(qkv[:, d:d + dkv])
    check_rows(kc, slice(pos, pos + 1), wq.view(B, 1, dkv), we.view(B, 1, dkv // 32), "kv8_rope_append rotate=False k")


@pytest.mark.parametrize("dkv,hd", GEOS)
def test_token_step_append_real_angles(dev, dkv, hd):
    """Position 37 of the default RoPE.  The kernel rotates in fp32 on the fp32 table the engine uses (ops.rope_table); against the float64
    rotation by the float64 angle an output a c - b s is off by at most (|a| + |b|) x (the table's error, bars.rope_angle_bar, + 4 x 2^-24 for the
    two products and the sum, half an ulp each, rounded up).  The stored k is then within half an e4m3 ulp at the element's scaled magnitude
    of that, v's exponents and codes are the rule's, the exponents of k equal the float64 row's wherever no block maximum is within the bar of
    a power of two (asserted of the inputs first, on the CPU), and q is within one rounding to bf16 (bars.BF16_OUT_REL) + the same bar."""
    B, Tmax, pos = 3, 40, 37
    Hkv = dkv // hd
    H = 2 * Hkv
    d = H * hd
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, d + 2 * dkv, generator=g).to(BF)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    ang = pos * inv
    # a block maximum above 448 / 512 of its power of two saturates, which no rounding bar covers (the exact-table test has that case): shrink
    # the raw partner blocks (32 j .. and the 32 at + hd/2, which the rotation mixes) of any such block until the rotated row has none
    for _ in range(64):
        m, _ = torch.frexp(rotate64(qkv[:, d:d + dkv], ang.cos(), ang.sin(), Hkv, hd).abs().view(B, Hkv, 2, hd // 64, 32).amax(-1))
        bad = (m >= 0.85).any(2, keepdim=True)
        if not bool(bad.any()):
            break
        raw = qkv[:, d:d + dkv].view(B, Hkv, 2, hd // 64, 32)
        raw.copy_(torch.where(bad[..., None], raw.float() * 0.8125, raw.float()).to(BF))
    rel = Bar.rope_angle_bar(ang) + 4.0 * Bar.U32                # per frequency, relative to |a| + |b| of the pair
    mag = lambda x, heads: x.double().abs().view(B, heads, 2, hd // 2).sum(2, keepdim=True).expand(-1, -1, 2, -1)  # noqa: E731
    k64 = rotate64(qkv[:, d:d + dkv], ang.cos(), ang.sin(), Hkv, hd)
    k_bar = (mag(qkv[:, d:d + dkv], Hkv) * rel).reshape(B, dkv)
    q64 = rotate64(qkv[:, :d], ang.cos(), ang.sin(), H, hd)
    q_bar = (mag(qkv[:, :d], H) * rel).reshape(B, d)
    # the inputs: no block maximum of the float64 k within its bar of a power of two, and none that saturates (448 / 256 of it and above)
    blocks = k64.abs().view(B, dkv // 32, 32)
    amax, at = blocks.max(-1)
    amax_bar = k_bar.view(B, dkv // 32, 32).gather(-1, at[..., None])[..., 0]
    m, _ = torch.frexp(amax)                                      # amax = m 2^e, m in [0.5, 1)
    assert bool(((m - 0.5) * 2 * amax > amax_bar).all()) and bool(((1.0 - m) * 2 * amax > amax_bar).all()) and bool((m < 448.0 / 512.0 - 1e-3).all())
    wq64, we64 = R8.mx_quantize64(k64)
    tab = ops.rope_table(1, hd, pos0=pos).view(hd // 2, 2)
    kc, vc = sentinel_caches(B, Tmax, dkv)
    gd = qkv.to(dev)
    ops.kv8_rope_append_(gd, H, Hkv, hd, tab, kc, vc, pos=pos)
    q_err = (gd[:, :d].double().cpu() - q64).abs()
    assert bool((q_err <= Bar.BF16_OUT_REL * q64.abs() + q_bar).all()), f"q: worst {float((q_err / (Bar.BF16_OUT_REL * q64.abs() + q_bar)).max()):.2f}x"
    wq, we = mx_bytes(qkv[:, d + dkv:])
    check_rows(vc, slice(pos, pos + 1), wq.view(B, 1, dkv), we.view(B, 1, dkv // 32), "v")
    kq, ke = (t.cpu() for t in ops.kv8_unpack(kc))
    assert torch.equal(ke[:, pos].int() - 127, we64), "k exponents"
    stored = R8.mx_dequantize64(kq[:, pos], we64)
    # half an e4m3 ulp at the element's scaled magnitude y = k 2^-e: the step is 2^(floor(log2 |y|) - 3), 2^-9 below the smallest normal 2^-6
    _, ey = torch.frexp(torch.ldexp(k64.view(B, dkv // 32, 32), -we64[..., None]).abs())
    half = 0.5 * torch.ldexp(torch.ones((), dtype=torch.float64), (ey - 1).clamp_min(-6) - 3 + we64[..., None]).view(B, dkv)
    err = (stored - k64).abs()
    print(f"RATIO kv8 k real angles {float((err / (half + k_bar)).max()):.3f}")
    assert bool((err <= half + k_bar).all())
    keep = [t for t in range(Tmax) if t != pos]
    assert bool((kq[:, keep] == SENT).all()) and bool((ke[:, keep] == SENT).all())


def decode_case(B, H, Hkv, hd, Tk, fam):
    """q and the MX images of the family's K and V (rows past Tk: code 0x7F, exponent 0xFF, both NaN) + the float64 reference on the dequantised
    values and its bar."""
    q, k, v, _ = A.make_inputs(fam, B, 1, Tk, H, Hkv, hd, False)
    Tmax, dkv = Tk + 3, Hkv * hd
    imgs, deq = [], []
    for x in (k, v):
        cq, ce = mxfp8.quantize(x.float())
        deq.append(mxfp8.dequantize(cq, ce))
        codes = torch.full((B, Tmax, dkv), 0x7F, dtype=torch.uint8)
        exps = torch.full((B, Tmax, dkv // 32), 0xFF, dtype=torch.uint8)
        codes[:, :Tk], exps[:, :Tk] = cq.view(B, Tk, dkv), (ce + 127).to(torch.uint8).view(B, Tk, dkv // 32)
        imgs.append(ops.kv8_pack(codes, exps))
    args = (B, 1, Tk, H, Hkv, hd, False, hd ** -0.5)
    o64 = A.attn_fwd64(q, deq[0], deq[1], *args)[0]
    if fam == "count":
        bar = Bar.attn_count_out_bar(o64, True)
    else:
        o32 = A.attn_fwd64(q, deq[0], deq[1], *args, dtype=torch.float32)[0]
        bar = Bar.attn_out_bar(o64, None, Bar.fp32_bar(o64, o32), True) + Bar.attn_decode_weight_term(Tk, deq[1])
    return q, imgs[0], imgs[1], o64, bar


# a trip of the kernel is 4 passes of 1024 / (hd / 16) rows: 512 rows at hd 128, 1024 at hd 64 -- one below, at, one above; with B * H > 1024 it is
# the 4-wave kernel and 4 passes of 256 / (hd / 16) rows: 128 rows at hd 128, 256 at hd 64
@pytest.mark.parametrize("fam", ["count", "offset"])
@pytest.mark.parametrize("B,H,Hkv,hd,Tk", [(2, 4, 4, 128, t) for t in (1, 64, 65, 257, 511, 512, 513)] + [(3, 8, 2, 64, t) for t in (1, 64, 65, 257, 1023, 1024, 1025)] +
                         [(17, 64, 8, 64, t) for t in (1, 255, 256, 257)] + [(9, 128, 16, 128, t) for t in (1, 127, 128, 129)])
def test_attention_over_the_image(dev, B, H, Hkv, hd, Tk, fam):
    q, kc, vc, o64, bar = decode_case(B, H, Hkv, hd, Tk, fam)
    qd, kd, vd = q.to(dev), kc.to(dev), vc.to(dev)
    o = ops.attention_decode_kv8(qd, kd, vd, H, Tk)
    check(o, o64, bar, f"decode kv8 B{B} H{H} Hkv{Hkv} hd{hd} Tk{Tk} {fam}", "decode-kv8 o")
    td = torch.tensor([Tk - 1], device=dev, dtype=torch.int32)
    assert torch.equal(ops.attention_decode_kv8(qd, kd, vd, H, 1, tk_dev=td), o)


def test_attention_clamps_a_device_length_to_the_cache(dev):
    """Tk + *tk_dev beyond Tmax reads the Tmax rows of the cache and nothing after them: the result of Tk = Tmax, bit for bit."""
    B, H, Hkv, hd, Tk = 2, 4, 2, 64, 70
    q, k, v, _ = A.make_inputs("randn", B, 1, Tk, H, Hkv, hd, False)
    imgs = []
    for x in (k, v):
        cq, ce = mx_bytes(x)
        imgs.append(ops.kv8_pack(cq.view(B, Tk, -1), ce.view(B, Tk, -1)).to(dev))
    want = ops.attention_decode_kv8(q.to(dev), imgs[0], imgs[1], H, Tk)
    td = torch.tensor([Tk + 7], device=dev, dtype=torch.int32)
    assert torch.equal(ops.attention_decode_kv8(q.to(dev), imgs[0], imgs[1], H, 1, tk_dev=td), want)


@pytest.mark.parametrize("dkv", [128, 512])
def test_gather_moves_codes_and_exponents_together(dev, dkv):
    """The prefix broadcast of a 2-row cache into 6 rows, then an in-place reorder of [t0, t1) by a parent map with a cycle (0 <- 1 <- 2 <- 0) and a
    parent taken twice (3): unpacked, dst[r] == src[parent[r]] byte for byte there and every other byte is what it was."""
    layers, T, S = 2, 7, 4
    g = torch.Generator().manual_seed(dkv)
    rnd = lambda *s: torch.randint(0, 256, s, generator=g, dtype=torch.uint8)  # noqa: E731
    src = [ops.kv8_pack(rnd(layers, 2, S, dkv), rnd(layers, 2, S, dkv // 32)).to(dev) for _ in range(2)]
    dst = [ops.kv8_pack(rnd(layers, 6, T, dkv), rnd(layers, 6, T, dkv // 32)).to(dev) for _ in range(2)]
    before = [[p.clone() for p in ops.kv8_unpack(t)] for t in dst]
    parent = (torch.arange(6, device=dev, dtype=torch.int32) // 3).contiguous()
    ops.kv8_gather_rows(src[0], src[1], dst[0], dst[1], parent, 0, S)
    for s, t, b in zip(src, dst, before):
        for ps, pt, pb in zip(ops.kv8_unpack(s), ops.kv8_unpack(t), b):
            assert torch.equal(pt[:, :, :S], ps[:, parent.long()]) and torch.equal(pt[:, :, S:], pb[:, :, S:])
    before = [[p.clone() for p in ops.kv8_unpack(t)] for t in dst]
    parent = torch.tensor([1, 2, 0, 3, 3, 4], device=dev, dtype=torch.int32)
    t0, t1 = 2, 5
    ops.kv8_gather_rows(dst[0], dst[1], dst[0], dst[1], parent, t0, t1)
    for t, b in zip(dst, before):
        for pt, pb in zip(ops.kv8_unpack(t), b):
            assert torch.equal(pt[:, :, t0:t1], pb[:, parent.long(), t0:t1])
            assert torch.equal(pt[:, :, :t0], pb[:, :, :t0]) and torch.equal(pt[:, :, t1:], pb[:, :, t1:])


def test_pack_unpack_roundtrip_cpu_side(dev):
    q = torch.arange(2 * 3 * 64, dtype=torch.int64).remainder(251).to(torch.uint8).view(2, 3, 64)
    e = torch.arange(2 * 3 * 2, dtype=torch.uint8).view(2, 3, 2)
    img = ops.kv8_pack(q.to(dev), e.to(dev))
    assert img.shape == (2, 3, 66) and img.dtype == torch.uint8
    uq, ue = ops.kv8_unpack(img)
    assert torch.equal(uq.cpu(), q) and torch.equal(ue.cpu(), e)
    assert torch.equal(img.view(-1)[:q.numel()].cpu(), q.view(-1)), "codes of all rows first, then the exponents"


def test_argument_refusals(dev):
    B, Tmax, dkv, hd = 2, 6, 128, 64
    kc, vc = sentinel_caches(B, Tmax, dkv)
    rows = torch.zeros(B * 4, 3 * dkv, device=dev, dtype=BF)
    with pytest.raises(ValueError, match="kv8_append"):
        ops.kv8_append(rows[:, dkv:2 * dkv], rows[:, 2 * dkv:], kc, vc, 4, Tmax - 3)                     # pos0 + T > Tmax
    qkv = torch.zeros(B, 4 * dkv, device=dev, dtype=BF)
    with pytest.raises(ValueError, match="kv8_rope_append"):
        ops.kv8_rope_append_(qkv, 8, 4, 32, torch.zeros(16, 2, device=dev), kc, vc, pos=0)              # head_dim 32
    q = torch.zeros(B, 2 * dkv, device=dev, dtype=BF)
    with pytest.raises(ValueError, match="attention_decode_kv8"):
        ops.attention_decode_kv8(q, kc, vc, 4, Tmax + 1)                                                 # a host length beyond the cache
    small = [ops.kv8_alloc(1, 2, 3, dkv=32) for _ in range(2)]
    with pytest.raises(ValueError, match="kv8_gather_rows"):
        ops.kv8_gather_rows(small[0], small[1], small[0], small[1], torch.zeros(2, device=dev, dtype=torch.int32), 0, 1)   # dkv % 64
    assert bool((ops.kv8_unpack(kc)[0] == SENT).all()), "a refused call writes nothing"
