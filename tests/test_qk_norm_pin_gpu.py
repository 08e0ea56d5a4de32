"""avllm_qk_norm_rope and avllm_qk_norm_bwd pinned elementwise to float64 (tests/refs64_qk_norm.py, bars: tests/bars_qk_norm.py, derived there and
from nothing a kernel returns), and avllm_dec_proj's raw_qkv form pinned to the bytes of the mode-0 launch on the same operands.  What the
kernels must not touch -- the v slice, the padding columns, every other cache row -- is compared as bytes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars  # noqa: E402
import bars_qk_norm as QB  # noqa: E402
import refs64_decode as D  # noqa: E402
import refs64_qk_norm as R  # noqa: E402
from avllm import ops  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32
SHAPES = ((48, 24, 0), (3, 1, 1000))                        # (rows, T, first position): 2 x 24 training rows; 3 single-token rows at a non-zero position


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bytes(a, b):
    return torch.equal(bits(a), bits(b))


def held(got, want, bar, tag):
    err = (got.double().cpu() - want).abs()
    ratio = err / bar
    bad = int(ratio.argmax())
    assert bool((err <= bar).all()), f"{tag}: err {float(err.flatten()[bad]):.3e} over bar {float(bar.flatten()[bad]):.3e} at element {bad} of {tuple(err.shape)}"
    return float(ratio.max())


def case(fam, geo, M, T, pos0, dtype):
    H, Hkv, hd = geo
    x, (wq, wk) = R.inputs(fam, M, H, Hkv, hd, dtype), R.weights(fam, hd, dtype)
    return x, wq, wk, R.table(T, hd, pos0)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("geo", R.GEOMETRY, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_forward_in_place_with_saves(dev, fam, geo, dtype):
    H, Hkv, hd = geo
    NQK, used = H + Hkv, (H + Hkv) * hd
    for M, T, pos0 in SHAPES:
        x, wq, wk, tab = case(fam, geo, M, T, pos0, dtype)
        ref = R.fwd64(x, H, Hkv, hd, wq, wk, R.EPS, tab)
        xd = x.to(dtype).cuda()
        x0 = xd.clone()
        pre, rstd = ops.qk_norm_rope_(xd, T, H, Hkv, hd, wq.to(dtype).cuda(), wk.to(dtype).cuda(), R.EPS, tab.cuda(), save=True)
        assert same_bytes(xd[:, used:], x0[:, used:]), "the v slice or the padding columns were written"
        assert same_bytes(pre, x0[:, :used]), "the saved pre-norm copy is not the input"
        w_out = held(xd[:, :used], ref.out, QB.fwd_bar(ref, dtype == BF), f"{fam} {geo} M={M} out")
        w_rs = held(rstd, ref.rstd, QB.rstd_bar(ref, dtype == F32), f"{fam} {geo} M={M} rstd")
        print(f"fwd {fam} {geo} {dtype} M={M}: worst err/bar out {w_out:.3e}, rstd {w_rs:.3e}")
        plain = x0.clone()                                  # without the saves: the same bytes
        ops.qk_norm_rope_(plain, T, H, Hkv, hd, wq.to(dtype).cuda(), wk.to(dtype).cuda(), R.EPS, tab.cuda())
        assert same_bytes(plain, xd)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("geo", R.GEOMETRY, ids=lambda g: "x".join(map(str, g)))
def test_cache_form(dev, geo, dtype):
    """k rows land rotated at pos + *pos_dev, v rows unrotated, every other cache row and the k | v | padding columns of the buffer keep their
    bytes, q is rewritten in the buffer; with pos + *pos_dev == Tmax nothing reaches the cache and q is still produced."""
    H, Hkv, hd = geo
    M, Tmax, dq, dkv = 3, 8, H * hd, Hkv * hd
    for fam in ("gauss", "locate"):
        x, wq, wk, tab = case(fam, geo, M, 1, 1000, dtype)
        ref = R.fwd64(x, H, Hkv, hd, wq, wk, R.EPS, tab)
        bar = QB.fwd_bar(ref, dtype == BF)
        wqd, wkd, tabd = wq.to(dtype).cuda(), wk.to(dtype).cuda(), tab.cuda()
        inplace = x.to(dtype).cuda()
        ops.qk_norm_rope_(inplace, 1, H, Hkv, hd, wqd, wkd, R.EPS, tabd)
        for pos, pos_dev, row in ((2, 3, 5), (7, None, 7), (5, 3, None), (8, 0, None)):
            kc = torch.randn(M, Tmax, dkv, generator=R.gen("kc", geo)).to(dtype).cuda()
            vc = torch.randn(M, Tmax, dkv, generator=R.gen("vc", geo)).to(dtype).cuda()
            kc0, vc0 = kc.clone(), vc.clone()
            xd = x.to(dtype).cuda()
            x0 = xd.clone()
            pd = None if pos_dev is None else torch.tensor([pos_dev], dtype=torch.int32, device="cuda")
            ops.qk_norm_rope_(xd, 1, H, Hkv, hd, wqd, wkd, R.EPS, tabd, kc=kc, vc=vc, pos=pos, pos_dev=pd)
            tag = f"{fam} {geo} pos {pos}+{pos_dev}"
            held(xd[:, :dq], ref.out[:, :dq], bar[:, :dq], tag + " q")
            assert same_bytes(xd[:, :dq], inplace[:, :dq]) and same_bytes(xd[:, dq:], x0[:, dq:]), tag
            keep = [t for t in range(Tmax) if t != row]
            assert same_bytes(kc[:, keep], kc0[:, keep]) and same_bytes(vc[:, keep], vc0[:, keep]), tag + ": another cache row was written"
            if row is not None:
                held(kc[:, row], ref.out[:, dq:], bar[:, dq:], tag + " k")
                assert same_bytes(kc[:, row], inplace[:, dq:dq + dkv]), tag + ": the cache row is not the in-place form's k"
                assert same_bytes(vc[:, row], x0[:, dq + dkv:dq + 2 * dkv]), tag + ": the v row is not the buffer's v"


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("geo", R.GEOMETRY, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("fam", R.FAMILIES + ("radial",))
def test_backward_in_place(dev, fam, geo, dtype):
    H, Hkv, hd = geo
    NQK, used, M, rounded = H + Hkv, (H + Hkv) * hd, 48, dtype == BF
    base = "gauss" if fam == "radial" else fam
    x, (wq, wk) = R.inputs(base, M, H, Hkv, hd, dtype), R.weights(base, hd, dtype)
    pre = x[:, :used].contiguous()
    rstd = R.fwd64(x, H, Hkv, hd, wq, wk, R.EPS, R.table(24, hd, 0), F32).rstd      # an input of the kernel and of the restatement alike
    dy = R.inputs(base, M, H, Hkv, hd, dtype, "dy")
    if fam == "radial":
        dyq, wq, wk = R.radial(pre, rstd, H, Hkv, hd)
        dy = torch.cat([dyq, dy[:, used:]], 1)
    r64, r32 = R.bwd64(dy, pre, rstd, H, Hkv, hd, wq, wk), R.bwd64(dy, pre, rstd, H, Hkv, hd, wq, wk, F32)
    bar = QB.radial_bar(r64, hd, rounded) if fam == "radial" else QB.bwd_bar(r64, r32, rounded)
    dyd = dy.to(dtype).cuda()
    dy0 = dyd.clone()
    ops.qk_norm_bwd_(dyd, H, Hkv, hd, wq.to(dtype).cuda(), wk.to(dtype).cuda(), pre.to(dtype).cuda(), rstd.cuda())
    assert same_bytes(dyd[:, used:], dy0[:, used:]), "the v slice or the padding columns of dqkv were written"
    w = held(dyd[:, :used], r64.dx, bar, f"bwd {fam} {geo}")
    print(f"bwd {fam} {geo} {dtype}: worst err/bar {w:.3e}; max |dx| {float(r64.dx.abs().max()):.3e}")


# ------------------------------------------------------------------------------------------------ dec_proj with raw_qkv
RAW_GEO = ((512, 128, 4, 2), (896, 64, 14, 2))             # (K, hd, heads, kv heads): the two fixture models' q|k|v projections


def dev_args(c):
    kw = dict(norm_w=c["g"].to(BF).cuda(), eps=c["eps"])
    if c.get("bias") is not None:
        kw["bias"] = c["bias"].to(BF).cuda()
    if c.get("lt") is not None:
        kw.update(lora_t=c["lt"].cuda(), lora_b=[b.to(BF).cuda() for b in c["lbs"]], lora_r=c["r"], lora_scale=c["scale"])
    return kw


@pytest.mark.parametrize("form", D.FORMS)
@pytest.mark.parametrize("geo", RAW_GEO, ids=lambda g: "x".join(map(str, g)))
def test_raw_qkv_is_the_plain_launch(dev, geo, form):
    """Without adapters: mode 2 with raw_qkv writes, bit for bit, what the mode-0 launch of the same rows on the same operands writes (the norm
    fold and the bias included), into a buffer whose rows are longer than N, and nothing else.  With adapters (mode 0 takes one module, mode
    2 three): the float64 restatement with the rotation switched off (cos 1, sin 0), under bars.dec_proj_bar."""
    K, hd, heads, kvh = geo
    dq, dkv = heads * hd, kvh * hd
    N = dq + 2 * dkv
    unit = torch.tensor([1.0, 0.0]).repeat(hd // 2, 1).contiguous()
    for M in (1, 5, 16):
        for lora, bias in ((False, False), (False, True), (True, False), (True, True)):
            c = D.qkv_case("randn", M, K, hd, heads, kvh, lora, bias)
            wa = D.wargs(c["W"], form)
            Wd = wa.pop("W")
            A = c["A"].to(BF).cuda()
            out = torch.full((M, N + 16), 7.0, dtype=BF, device="cuda")
            ops.dec_proj(A, Wd, mode=2, out=out[:, :N], dq=dq, dkv=dkv, hd=hd, raw_qkv=True, **dev_args(c), **wa)
            assert bool((out[:, N:] == 7.0).all()), "columns past N were written"
            tag = f"raw {geo} {form} M={M} lora={lora} bias={bias}"
            if not lora:
                plain = ops.dec_proj(A, Wd, mode=0, **dev_args(c), **wa)
                assert same_bytes(out[:, :N], plain), tag
            ref = D.dec_proj64(**dict(c, rope=unit))
            err = (out[:, :N].double().cpu() - ref.out).abs()
            assert bool((err <= bars.dec_proj_bar(ref)).all()), tag
