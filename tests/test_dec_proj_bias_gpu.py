"""The bias term of avllm_dec_proj (Qwen2's q|k|v bias, attention_bias' o bias on the fused token step) against float64.  Families as in
test_gemm_pin_gpu.py: `locate` (zero weights, bias[n] = a distinct small integer per column: a column that takes another column's bias, which
the permuted column order of the rotary region invites, is a wrong integer) and `exact` (operands on grids where every partial sum is exact)
carry the bar 0; `offset` (bias +-64 on products of size 1: the Qwen case, k biases are large) is held to ONE rounding of the exact sum by
bars.gemm_bar.  Bars come from tests/bars.py unchanged."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars  # noqa: E402
import mxfp4_ref as mx4  # noqa: E402
import refs64_gemm as G  # noqa: E402
from avllm import ops  # noqa: E402
from refs64_decode import distinct_bias, gen, grid_weights, ints, rope_table, rot, wargs  # noqa: E402

BF, F64 = torch.bfloat16, torch.float64
FORMS = ("bf16", "fp8", "fp4")


# ------------------------------------------------------------------------------------------------ locate, bar 0
@pytest.mark.parametrize("K", [128, 896, 1152])
@pytest.mark.parametrize("M", [1, 5, 16])
def test_locate_plain(dev, M, K):
    """mode 0 over zero weights: every output column is its own bias, with and without the norm fold, the residual and adapters."""
    N, r = 512, 8
    A = torch.randn(M, K, generator=gen("a", M, K)).to(BF).cuda()
    W = torch.zeros(N, K, dtype=BF, device=dev)
    b = distinct_bias(N)
    bias = b.to(BF).cuda()
    g = (1.0 + 0.1 * torch.randn(K, generator=gen("g", K))).to(BF).cuda()
    want = b[None, :].expand(M, N)
    assert torch.equal(ops.dec_proj(A, W, bias=bias).float().cpu(), want)                       # bf16 output: the integers are bf16 values
    assert torch.equal(ops.dec_proj(A, W, bias=bias, out_f32=True).cpu(), want)
    assert torch.equal(ops.dec_proj(A, W, bias=bias, norm_w=g, eps=1e-6, out_f32=True).cpu(), want)
    R = ints((M, N), -3, 3, "r", M)
    lt = torch.zeros(M, 64)
    lt[:, :r] = ints((M, r), -2, 2, "lt", M)
    lb = torch.zeros(N, 64)
    lb[:, :r] = ints((N, r), -2, 2, "lb")
    out = ops.dec_proj(A, W, bias=bias, R=R.to(BF).cuda(), out_f32=True)
    assert torch.equal(out.cpu(), want + R)
    out = ops.dec_proj(A, W, bias=bias, R=R.to(BF).cuda(), out_f32=True, lora_t=lt.cuda(), lora_b=[lb.to(BF).cuda()], lora_r=r, lora_scale=2.0)
    assert torch.equal(out.cpu(), want + R + 2.0 * (lt @ lb.t()))


@pytest.mark.parametrize("hd,heads,kvh", [(64, 4, 2), (128, 2, 1)])
@pytest.mark.parametrize("K", [128, 896, 1152])
@pytest.mark.parametrize("M", [1, 5, 16])
def test_locate_qkv(dev, M, K, hd, heads, kvh):
    """mode 2 over zero weights.  Rope table (cos 1, sin 0): q and the cache rows at `pos` are the bias; (cos 0, sin 1): the first half of every
    head is minus its partner's bias, the second half plus.  In the rotary region the kernel's columns are permuted (8 columns of a head's
    first half next to their 8 partners): the bias is indexed by the logical column, and this is where it would go wrong."""
    dq, dkv, Tmax, pos, r = heads * hd, kvh * hd, 5, 3, 8
    N = dq + 2 * dkv
    A = torch.randn(M, K, generator=gen("a", M, K)).to(BF).cuda()
    W = torch.zeros(N, K, dtype=BF, device=dev)
    b = distinct_bias(N)
    bias = b.to(BF).cuda()
    g = (1.0 + 0.1 * torch.randn(K, generator=gen("g", K))).to(BF).cuda()
    rows = b[None, :].expand(M, N).contiguous()
    lt = torch.zeros(M, 192)
    Bs, add = [], torch.zeros(M, N)
    off = 0
    for j, w in enumerate((dq, dkv, dkv)):
        lt[:, 64 * j:64 * j + r] = ints((M, r), -1, 1, "lt", j, M)
        lb = torch.zeros(w, 64)
        lb[:, :r] = ints((w, r), -1, 1, "lb", j)
        lb[b[off:off + w].abs() > 240] = 0                    # |bias + adapter term| stays <= 256, where every integer is a bf16 value
        add[:, off:off + w] = lt[:, 64 * j:64 * j + r] @ lb[:, :r].t()
        Bs.append(lb.to(BF).cuda())
        off += w
    for (c, s) in ((1.0, 0.0), (0.0, 1.0)):
        for lora in (False, True):
            y = rows + add if lora else rows
            kw = dict(lora_t=lt.cuda(), lora_b=Bs, lora_r=r, lora_scale=1.0) if lora else {}
            kc = torch.full((M, Tmax, dkv), 7.0, device=dev, dtype=BF)
            vc = torch.full((M, Tmax, dkv), -7.0, device=dev, dtype=BF)
            q = ops.dec_proj(A, W, mode=2, norm_w=g, eps=1e-6, rope=rope_table(hd, c, s), kc=kc, vc=vc, pos=pos, dq=dq, dkv=dkv, hd=hd, bias=bias, **kw)
            wq, wk, wv = rot(y[:, :dq], heads, hd, c, s), rot(y[:, dq:dq + dkv], kvh, hd, c, s), y[:, dq + dkv:]
            for t in (wq, wk, wv):
                assert torch.equal(t.to(BF).float(), t)        # the expected integers are bf16 values: bar 0 on a bf16 output
            assert torch.equal(q.float().cpu(), wq), (c, s, lora)
            assert torch.equal(kc[:, pos].float().cpu(), wk), (c, s, lora)
            assert torch.equal(vc[:, pos].float().cpu(), wv), (c, s, lora)
            keep = [t for t in range(Tmax) if t != pos]
            assert (kc[:, keep] == 7.0).all() and (vc[:, keep] == -7.0).all()


# ------------------------------------------------------------------------------------------------ exact, bar 0, three weight forms
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("K", [128, 896, 1152])
@pytest.mark.parametrize("M", [1, 5, 16])
def test_exact_sum_with_bias(dev, M, K, form):
    """Small-integer activations and bias on grid weights: every product and partial sum is a multiple of 2^-4 below 2^20, exact in fp32 in any
    order, so the f32 output IS the float64 sum, in every weight form, with the residual and adapters on top."""
    N, r = 48, 8
    W = grid_weights(N, K)
    A = ints((M, K), -2, 2, "a", M, K)
    b = ints((N,), -100, 100, "b", K)
    R = ints((M, N), -5, 5, "r", M)
    ref = (A.double() @ W.double().t() + b.double()[None, :])
    assert float(ref.abs().max()) < 2.0 ** 20 and float((A.abs().double() @ W.abs().double().t()).max()) < 2.0 ** 20
    wa = wargs(W, form)
    Wd = wa.pop("W")
    out = ops.dec_proj(A.to(BF).cuda(), Wd, bias=b.to(BF).cuda(), out_f32=True, **wa)
    assert torch.equal(out.cpu().double(), ref)
    lt = torch.zeros(M, 64)
    lt[:, :r] = ints((M, r), -2, 2, "lt", M)
    lb = torch.zeros(N, 64)
    lb[:, :r] = ints((N, r), -2, 2, "lb")
    out = ops.dec_proj(A.to(BF).cuda(), Wd, bias=b.to(BF).cuda(), R=R.to(BF).cuda(), out_f32=True, lora_t=lt.cuda(), lora_b=[lb.to(BF).cuda()],
                       lora_r=r, lora_scale=0.5, **wa)
    assert torch.equal(out.cpu().double(), ref + R.double() + 0.5 * (lt.double() @ lb.double().t()))


# ------------------------------------------------------------------------------------------------ offset: one rounding of the exact sum
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M", [1, 5, 16])
def test_offset_bias_is_added_before_the_one_rounding(dev, M, form):
    """bias = +-64 on products of size ~1, bf16 output: the result is held to one rounding of the exact sum plus the fp32 accumulator's bound
    (bars.gemm_bar, kind split8: 8 wave partials met in LDS), 2^-8 |out| = 0.25 at this size.  A bias of the neighbouring column (the signs
    alternate) is 128 away, a missing one 64; at this offset the bar is the result's own last place and cannot be tightened further."""
    K, N = 896, 64
    W = mx4.dequantize(*mx4.quantize(torch.randn(N, K, generator=gen("w")) * K ** -0.5))       # values all three forms hold
    A = torch.randn(M, K, generator=gen("a", M)).to(BF)
    b = 64.0 * (1.0 - 2.0 * (torch.arange(N) % 2)).float()
    ref = G.gemm(A.float(), W, bias=b)
    assert 0.3 < float(ref.acc.abs().mean()) < 3.0
    bar = bars.gemm_bar(ref, K, "split8")
    wa = wargs(W, form)
    out = ops.dec_proj(A.cuda(), wa.pop("W"), bias=b.to(BF).cuda(), **wa)
    err = (out.cpu().double() - ref.out).abs()
    print(f"offset {form} M={M}: max err {float(err.max()):.3e}, bar at that element {float(bar.flatten()[err.argmax()]):.3e}")
    assert bool((err <= bar).all())


@pytest.mark.parametrize("hd,heads,kvh", [(64, 4, 2), (128, 2, 1)])
def test_offset_qkv_identity_rope(dev, hd, heads, kvh):
    """The same through mode 2: rope (1, 0) is the identity, so q and the cache rows are the once-rounded sums."""
    M, K = 5, 896
    dq, dkv = heads * hd, kvh * hd
    N = dq + 2 * dkv
    W = (torch.randn(N, K, generator=gen("wq", hd)) * K ** -0.5).to(BF)
    A = torch.randn(M, K, generator=gen("aq", hd)).to(BF)
    b = 64.0 * (1.0 - 2.0 * ((torch.arange(N) // 3) % 2)).float()
    kc = torch.zeros(M, 2, dkv, device=dev, dtype=BF)
    vc = torch.zeros_like(kc)
    q = ops.dec_proj(A.cuda(), W.cuda(), mode=2, rope=rope_table(hd, 1.0, 0.0), kc=kc, vc=vc, pos=1, dq=dq, dkv=dkv, hd=hd,
                     bias=b.to(BF).cuda())
    got = torch.cat([q, kc[:, 1], vc[:, 1]], 1).cpu().double()
    ref = G.gemm(A.float(), W.float(), bias=b)
    err = (got - ref.out).abs()
    assert bool((err <= bars.gemm_bar(ref, K, "split8")).all()), float(err.max())


# ------------------------------------------------------------------------------------------------ refusals, the bias-free launch
def test_swiglu_with_a_bias_is_refused(dev):
    A = torch.randn(4, 256, generator=gen("a")).to(BF).cuda()
    W = torch.randn(128, 256, generator=gen("w")).to(BF).cuda()
    with pytest.raises(ValueError, match="SwiGLU"):
        ops.dec_proj(A, W, mode=1, bias=torch.zeros(64, dtype=BF, device=dev))
    ops.dec_proj(A, W, mode=1)
    with pytest.raises(ValueError):
        ops.dec_proj(A, W, bias=torch.zeros(128, dtype=torch.float32, device=dev))       # bf16 only
    with pytest.raises(ValueError):
        ops.dec_proj(A, W, bias=torch.zeros(64, dtype=BF, device=dev))                   # [N]


def null_bias_cases(form, dev="cuda"):
    """[(keyword arguments, output)] of bias-free launches on fixed inputs: f32 out, residual, norm fold.  Uses no argument the library lacked
    before the bias existed, so the same function records the checksums below on the commit before it."""
    M, K, N = 5, 1152, 64
    W = mx4.dequantize(*mx4.quantize(torch.randn(N, K, generator=gen("w0")) * K ** -0.5))
    A = torch.randn(M, K, generator=gen("a0")).to(BF).cuda()
    R = torch.randn(M, N, generator=gen("r0")).to(BF).cuda()
    wa = wargs(W, form)
    Wd = wa.pop("W")
    kws = (dict(out_f32=True), dict(R=R), dict(norm_w=torch.ones(K, dtype=BF, device=dev), eps=1e-5))
    return A, Wd, wa, [(kw, ops.dec_proj(A, Wd, **kw, **wa)) for kw in kws]


def checksum(outs):
    import hashlib
    h = hashlib.sha256()
    for _, o in outs:
        h.update(o.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


# sha256 over the three outputs' bytes, recorded by running null_bias_cases on the commit before the bias term existed (MI355X).
# These pin the fp32 summation order of dec_proj.  A later change that moves it on purpose re-records them with
# tools/record_dec_proj_null_sha.py pointed at a build of the PARENT of that change, and shows by the same run on its own tree that a launch
# without a bias still equals a zero bias; hashes taken from the changed tree itself would prove nothing.
NULL_BIAS_SHA = {
    "bf16": "6e317a4e65b7291e3860f8836a36d33a08ff32063e3a22eb8350cdcfab2dff58",
    "fp8": "c7ffeabc2e2e39b4804aef1b8ec4ee77703a75496e8f7149a23412025e882b76",
    "fp4": "4654927c7ba0ba4cf7e9b8152983989a2fe600258fcdf4fdd26eae662255d817",
}


@pytest.mark.parametrize("form", FORMS)
def test_null_bias_is_the_launch_it_always_was(dev, form):
    """No bias: bit for bit the bytes the library wrote before it knew the term; a zero bias: the same values."""
    A, Wd, wa, outs = null_bias_cases(form)
    assert checksum(outs) == NULL_BIAS_SHA[form]
    for kw, a in outs:
        z = ops.dec_proj(A, Wd, bias=torch.zeros(a.shape[1], dtype=BF, device=dev), **kw, **wa)
        assert torch.equal(a, z)
