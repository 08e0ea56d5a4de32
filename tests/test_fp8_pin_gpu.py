"""The block-scaled fp8 kernels (csrc/fp8.hip: mx_quant_kernel, gemm_f8_ref_kernel, norm_mxq_kernel; csrc/fp8_fast.hip: gemm_f8_wp_kernel) against the
float64 restatements of tests/refs64_fp8.py.  Bars: tests/bars.py ("block-scaled fp8 against float64"); none is taken from a kernel's output, and
tests/test_fp8_refs_cpu.py checks the references, the families' premises and the quantised-output rules on the host.

Every GEMM call first asserts the kernel ops.gemm_f8(..., plan=True) names.  Codes travel as column slices of wider buffers whose padding holds the
e4m3 NaN code (lda, ldb > K), C is a view (row 1, column 8 on) of a larger NaN buffer with ldc > N and spare rows, R a slice of a buffer of yet
another width: afterwards everything outside C must still be NaN and everything inside written.  The zero-bar families reach the kernel as hand-made
codes and scale images (refs64_fp8.encode_image), never through the quantiser; the barred ones are quantised by avllm_mx_quantize from strided
inputs and referenced from the codes and the whole image read back; their accumulator bar carries what the scaled MFMA drops inside its groups of
8 products (refs64_fp8.mfma_group_loss, measured and derived in bars.py), computed from those codes.  Each case prints "RATIO kernel family o(bf16|f32) act worst"."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64_fp8 as F8  # noqa: E402
import refs64_gemm as G  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402
from oracle import mxfp8 as MX  # noqa: E402
from test_gemm_pin_gpu import C0, R0, dev_, note, report  # noqa: E402

F64, F32, BF16, U8 = torch.float64, torch.float32, torch.bfloat16, torch.uint8
NAN_CODE = 0x7F
REFUSED = (ValueError, L.AvllmError)


@pytest.fixture(autouse=True)
def stop_after_a_gpu_fault():
    """A failed comparison is a finding; a device fault is not something to keep launching kernels after: it ends the session."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"the GPU reported {err}: nothing more is launched", returncode=3)


def slice_of(t, dtype, fill, left=16, extra=32):
    """t [rows, cols] -> the same values as a column slice (offset `left`, row stride cols + extra) of a buffer filled with `fill`, on the GPU."""
    wide = torch.full((t.shape[0], t.shape[1] + extra), fill, device="cuda", dtype=dtype)
    view = wide[:, left:left + t.shape[1]]
    view.copy_(t.to(dtype))
    return view


# ------------------------------------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=3)
def zero_operand(fam, M, N, K, wide=True):
    d = F8.zero_family(fam, M, N, K, wide)
    assert F8.zero_exact(d, 1.0 if fam == "intsum" else 2.0 ** -4)
    acc = F8.zero_product(d)
    return dict(Aq=slice_of(d["Aq"], U8, NAN_CODE), As=F8.encode_image(d["Ae"], 0, M, K).cuda(), Bq=slice_of(d["Bq"], U8, NAN_CODE),
                Bs=F8.encode_image(d["Be"], 1, N, K).cuda(), bias=d["bias"], R=d["R"], acc=acc, acc_d=acc.cuda().double())


def quantised(x, layout):
    """x fp32 [R, K] of bf16 values -> (codes view with ld > K on the GPU, image on the GPU, codes on the host, exponents read back from the WHOLE
    image); the input is a column slice too (ldx > K) and the padded bytes of the image must be zero."""
    R, K = x.shape
    xs = slice_of(x, BF16, float("nan"), left=8, extra=24)
    q = torch.full((R, K + 32), NAN_CODE, device="cuda", dtype=U8)[:, 16:16 + K]
    _, s = ops.mx_quantize(xs, layout, q=q)
    e, pad = F8.read_image(s, layout, R, K)
    assert int(pad.count_nonzero()) == 0, "padded bytes of the scale image"
    return q, s, q.cpu(), e


@functools.lru_cache(maxsize=3)
def barred_operand(fam, M, N, K, sampled):
    d = F8.barred_family(fam, M, N, K)
    Aq, As, Ah, Ae = quantised(d["A"], 0)
    Bq, Bs, Bh, Be = quantised(d["W"], 1)
    rows = G.sample_rows(M) if sampled else torch.arange(M)
    loss = F8.mfma_group_loss(Ah[rows].cuda(), Ae[rows].cuda(), Bh.cuda(), Be.cuda())          # what the instruction may drop inside its groups of 8 (bars.py)
    return dict(Aq=Aq, As=As, Bq=Bq, Bs=Bs, bias=d["bias"], R=d["R"], rows=rows, a64=F8.decode(Ah[rows], Ae[rows]), b64=F8.decode(Bh, Be), loss=loss)


# ------------------------------------------------------------------------------------------------ one launch, one check
def launch(op, M, N, kernel, rows, want, bar, bias=None, R=None, act=0, inplace=False):
    """Plan, run into a fresh NaN buffer, verify.  rows: the output rows `want` (float64 on the GPU) covers; the rest is only checked for having been
    written.  -> the failure text, or the worst error / bar."""
    ldc = (N + 7) // 8 * 8 + 16
    buf = torch.full((M + R0 + 3, ldc), float("nan"), device="cuda", dtype=BF16)
    out = buf[R0:R0 + M, C0:C0 + N]
    Rd = None
    if R is not None:
        Rd = slice_of(R, BF16, float("nan"), left=8, extra=ldc - N + 8)       # ldr = ldc + 8
        if inplace:
            out.copy_(Rd)
            Rd = out
    kw = dict(out=out, bias=dev_(bias, BF16), R=Rd, act=act)
    planned = ops.gemm_f8(op["Aq"], op["As"], op["Bq"], op["Bs"], plan=True, **kw)
    if planned != kernel:
        return f"planned on {planned}, not {kernel}"
    ops.gemm_f8(op["Aq"], op["As"], op["Bq"], op["Bs"], **kw)
    torch.cuda.synchronize()
    every = torch.arange(M, device="cuda")
    canary, unwritten, _ = G.verify(buf, R0, C0, every, N, out.double(), 0.0)            # NaN - NaN: an element left alone counts as beyond the bar
    _, over, ratio = G.verify(buf, R0, C0, rows.cuda(), N, want, bar)
    if canary or unwritten or over:
        return f"{over}/{want.numel()} beyond the bar (worst {ratio:.2f}x), {unwritten} never written, {canary} canaries overwritten"
    return ratio


def zero_cases(kernel, M, N, K, epis):
    """(what, failure or ratio) of both bf16 zero-bar families under every linear epilogue of `epis`."""
    every = torch.arange(M)
    for fam in F8.ZERO_BAR:
        for e in epis:
            if e.act:
                continue
            wide = fam == "selector" and not (e.bias or e.R)
            op = zero_operand(fam, M, N, K, wide)
            want = op["acc_d"]
            if e.bias:
                want = want + op["bias"].double().cuda()[None, :]
            if e.R:
                want = want + op["R"].double().cuda()
            assert torch.equal(want, want.to(BF16).to(F64))
            r = launch(op, M, N, kernel, every, want, 0.0, op["bias"] if e.bias else None, op["R"] if e.R else None, 0, e.inplace)
            yield f"{kernel} {M}x{N}x{K} {fam} {e.name}", fam, e, r


def barred_cases(kernel, M, N, K, epis, sampled):
    for fam in F8.BARRED:
        op = barred_operand(fam, M, N, K, sampled)
        rows = op["rows"]
        for e in epis:
            bias = op["bias"] if e.bias else None
            R = op["R"] if e.R else None
            if fam == "offset" and e.R:                                       # R = -z + noise on the checked rows: ONE bf16 rounding is all the bar allows
                R = R.clone()
                R[rows] = G.cancel_R(G.gemm(op["a64"], op["b64"], bias=bias, act=e.act).out, len(rows))
            ref = G.gemm(op["a64"], op["b64"], bias=bias, R=None if R is None else R[rows], act=e.act)
            ref = G.Ref(*(None if t is None else t.cuda() for t in ref))
            bar = Bar.fp8_gemm_bar(ref, K, e.act, True, op["loss"])
            assert bool(torch.isfinite(bar).all()) and bool((bar > 0).all())          # a NaN bar would pass every comparison
            r = launch(op, M, N, kernel, rows, ref.out, bar, bias, R, e.act, e.inplace)
            yield f"{kernel} {M}x{N}x{K} {fam} {e.name}", fam, e, r


def settle(kernel, results):
    bad, n = [], 0
    for what, fam, e, r in results:
        n += 1
        if isinstance(r, str):
            bad.append(f"{what}: {r}")
        else:
            note(kernel, fam, True, e.act, r)
    assert not bad, f"{len(bad)}/{n} calls failed:\n" + "\n".join(bad[:40])
    report((kernel,))


# ------------------------------------------------------------------------------------------------ the reference-grade kernel
@pytest.mark.parametrize("K", F8.REF_K)
@pytest.mark.parametrize("M", F8.REF_M)
def test_reference_grade_kernel(dev, M, K):
    def cases():
        for N in F8.REF_N:
            yield from zero_cases("ref", M, N, K, F8.EPIS)
            yield from barred_cases("ref", M, N, K, F8.EPIS, False)
    with L.knob("F8_FAST", 0):
        settle("ref", cases())


# ------------------------------------------------------------------------------------------------ the persistent kernel
@pytest.mark.parametrize("group", ("zero", "barred"))
@pytest.mark.parametrize("K", F8.FAST_K)
@pytest.mark.parametrize("M,N", F8.FAST_MN, ids=lambda v: str(v))
def test_fast_kernel(dev, M, N, K, group):
    settle("fast", zero_cases("fast", M, N, K, F8.EPIS) if group == "zero" else barred_cases("fast", M, N, K, F8.EPIS, True))


@pytest.mark.parametrize("group", ("zero", "barred"))
@pytest.mark.parametrize("K", F8.WALK_K)
@pytest.mark.parametrize("tm,tn", F8.WALK_TILES, ids=lambda v: str(v))
def test_fast_kernel_walk(dev, tm, tn, K, group):
    """24 x 22 = 528 tiles: every workgroup of a 256-CU part walks two tiles and 16 of them a third (the buffer parity and the relaxed wait after a
    full epilogue repeat; K = 384 flips the stage-buffer parity at every tile boundary); 17 x 16 = 272: 16 workgroups walk two."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if (tm, tn) == F8.WALK_TILES[0]:
        assert tm * tn > 2 * cus, f"{tm * tn} tiles: no workgroup of {cus} walks a third"
    else:
        assert tm * tn > cus
    M, N = tm * 256 - 3, tn * 256 - 8
    walk = tuple(e for e in F8.EPIS if e.name in ("plain", "bias_R", "gelu"))      # plain, bias + R, bias + act
    settle("fast-walk", zero_cases("fast", M, N, K, walk) if group == "zero" else barred_cases("fast", M, N, K, walk, True))


# ------------------------------------------------------------------------------------------------ quantised output
def q_launch(op, M, N, bias, act):
    assert ops.gemm_f8(op["Aq"], op["As"], op["Bq"], op["Bs"], bias=dev_(bias, BF16), act=act, quantised_out=True, plan=True) == "fast"
    q, sc = ops.gemm_f8(op["Aq"], op["As"], op["Bq"], op["Bs"], bias=dev_(bias, BF16), act=act, quantised_out=True)
    torch.cuda.synchronize()
    return q, sc


@pytest.mark.parametrize("K", F8.WALK_K)
@pytest.mark.parametrize("M,N", F8.QOUT_MN, ids=lambda v: str(v))
def test_quantised_output_intsum_is_bit_equal(dev, M, N, K):
    """The fp32 value before quantisation is an exact integer: codes and the WHOLE scale image (padded bytes and the rows >= M of the last group: zero)
    equal the rule applied on the host, with and without an integer bias."""
    op = zero_operand("intsum", M, N, K)
    for bias in (None, op["bias"]):
        z = op["acc"] if bias is None else op["acc"] + bias[None, :]
        codes, e = MX.quantize(z)
        q, sc = q_launch(op, M, N, bias, 0)
        wrong = int((q.cpu() != codes).sum())
        assert wrong == 0, f"{wrong} codes differ; first at {(q.cpu() != codes).nonzero()[:4].tolist()}"
        got_e, pad = F8.read_image(sc, 0, M, N)
        assert torch.equal(got_e, e), f"{int((got_e != e).sum())} exponents differ"
        assert int(pad.count_nonzero()) == 0 and torch.equal(sc.cpu(), F8.encode_image(e, 0, M, N))


@pytest.mark.parametrize("fam", F8.BARRED)
@pytest.mark.parametrize("K", F8.WALK_K)
@pytest.mark.parametrize("M,N", F8.QOUT_MN, ids=lambda v: str(v))
def test_quantised_output_within_half_a_step(dev, M, N, K, fam):
    """Every block's exponent in the admissible set, every element within step / 2 + bar under that exponent (refs64_fp8.quant_errors: no share
    exempted), for act in {none, gelu, quick_gelu, silu}; then the pair as the A operand of the next GEMM against the float64 product of THOSE codes.
    The two 2048-wide shapes are checked in full, the walk shape on sampled rows (all blocks of each)."""
    full = M * N <= 2048 * 2048
    op = barred_operand(fam, M, N, K, not full)
    rows = op["rows"]
    acc = (op["a64"] @ op["b64"].t()).cuda()
    sum_abs = (op["a64"].abs() @ op["b64"].abs().t()).cuda()
    z = acc + op["bias"].double().cuda()[None, :]
    W2 = F8.barred_family("randn", 8, 256, N)["W"]
    W2q, W2s, W2h, W2e = quantised(W2, 1)
    bad = []
    for act in F8.QOUT_ACTS:
        ref = G.Ref(G.act64(z, act), sum_abs, z, acc, None, None)
        bar = Bar.fp8_gemm_bar(ref, K, act, False, op["loss"])
        assert bool(torch.isfinite(bar).all()) and bool((bar > 0).all())
        q, sc = q_launch(op, M, N, op["bias"], act)
        e, pad = F8.read_image(sc, 0, M, N)
        assert int(pad.count_nonzero()) == 0
        blocks, over, ratio = F8.quant_errors(q[rows.cuda()], e[rows].cuda(), ref.out, bar)
        if blocks or over:
            bad.append(f"act {act}: {blocks} exponents outside the admissible set, {over}/{ref.out.numel()} elements beyond step / 2 + bar (worst {ratio:.3f}x)")
            continue
        note("fast-q", fam, False, act, ratio)
        if act in (0, 2):
            qr = q.cpu()[rows]
            ref2 = G.Ref(*(None if t is None else t.cuda() for t in G.gemm(F8.decode(qr, e[rows]), F8.decode(W2h, W2e))))
            loss2 = F8.mfma_group_loss(qr.cuda(), e[rows].cuda(), W2h.cuda(), W2e.cuda())
            buf = torch.full((M + R0 + 3, 256 + 16), float("nan"), device="cuda", dtype=BF16)
            ops.gemm_f8(q, sc, W2q, W2s, out=buf[R0:R0 + M, C0:C0 + 256])
            torch.cuda.synchronize()
            _, over2, r2 = G.verify(buf, R0, C0, rows.cuda(), 256, ref2.out, Bar.fp8_gemm_bar(ref2, N, 0, True, loss2))
            if over2:
                bad.append(f"act {act}: the pair as an A operand: {over2} beyond the bar (worst {r2:.2f}x)")
    assert not bad, "\n".join(bad)
    report(("fast-q",))


def test_quantised_output_refuses_a_partial_scale_plane(dev):
    """N % 128 != 0: the epilogue would write the scale plane of the last, partial 128-column group one plane past avllm_mx_scale_bytes(M, N).  The
    host refuses before any launch (2048 x 2080 is 72 tiles: everything else about the call is what the persistent kernel takes)."""
    M, N, K = 2048, 2080, 256
    Aq, Bq = torch.zeros(M, K, device="cuda", dtype=U8), torch.zeros(N, K, device="cuda", dtype=U8)
    As = torch.zeros(L.load().avllm_mx_scale_bytes(M, K), device="cuda", dtype=U8)
    Bs = torch.zeros(L.load().avllm_mx_scale_bytes(N, K), device="cuda", dtype=U8)
    assert ops.gemm_f8(Aq, As, Bq, Bs, plan=True) == "fast"
    assert ops.gemm_f8(Aq, As, Bq, Bs, quantised_out=True, plan=True) == "ref"
    q = torch.zeros(M, N, device="cuda", dtype=U8)
    sc = torch.zeros(L.load().avllm_mx_scale_bytes(M, N) + 65536, device="cuda", dtype=U8)          # room beyond the image: nothing may land there either
    d = L.GemmF8Desc()
    d.A, d.SA, d.B, d.SB, d.lda, d.ldb, d.M, d.N, d.K = L.ptr(Aq), L.ptr(As), L.ptr(Bq), L.ptr(Bs), K, K, M, N, K
    d.Cq, d.SCq, d.ldcq = L.ptr(q), L.ptr(sc), N
    assert L.load().avllm_gemm_f8_takes_quantised_output(C.byref(d)) == 0 and L.load().avllm_gemm_f8_takes_fast(C.byref(d)) == 0
    rc = L.load().avllm_gemm_f8(C.byref(d), L.stream_ptr())
    assert rc != 0 and "128" in L.load().avllm_last_error().decode()
    with pytest.raises(REFUSED):
        ops.gemm_f8(Aq, As, Bq, Bs, quantised_out=True)
    torch.cuda.synchronize()
    assert int(sc.count_nonzero()) == 0 and int(q.count_nonzero()) == 0
    d.N = 2048                                                                                        # the same call one partial group narrower is taken
    assert L.load().avllm_gemm_f8_takes_quantised_output(C.byref(d)) == 1


# ------------------------------------------------------------------------------------------------ the quantiser
def quantise_and_compare(x, layout, what):
    """x on the host, in its dtype -> codes and the ENTIRE image bit for bit against the rule and encode_image; then the s= form over an image that held
    other values."""
    R, K = x.shape
    codes, e = MX.quantize(x.float())
    img = F8.encode_image(e, layout, R, K)
    xs = slice_of(x, x.dtype, float("nan"), left=8, extra=24)                 # ldx > K
    qbuf = torch.full((R + 2, K + 32), 0x55, device="cuda", dtype=U8)
    q, s = ops.mx_quantize(xs, layout, q=qbuf[1:1 + R, 16:16 + K])
    torch.cuda.synchronize()
    bad = []
    if not torch.equal(q.cpu(), codes):
        at = (q.cpu() != codes).nonzero()[0].tolist()
        bad.append(f"{what}: {int((q.cpu() != codes).sum())} codes differ, first at {at}: x {float(x[at[0], at[1]]):.9g} -> {int(q[at[0], at[1]]):#x}, rule {int(codes[at[0], at[1]]):#x}")
    qbuf[1:1 + R, 16:16 + K] = 0x55
    if int((qbuf != 0x55).sum()):
        bad.append(f"{what}: codes stored outside [R, K]")
    if not torch.equal(s.cpu().reshape(-1), img):
        bad.append(f"{what}: {int((s.cpu().reshape(-1) != img).sum())} bytes of the scale image differ")
    s2 = torch.full_like(s, 0xAB)
    ops.mx_quantize(xs, layout, q=q, s=s2)
    if not torch.equal(s2.cpu().reshape(-1), img):
        bad.append(f"{what}: s= form: {int((s2.cpu().reshape(-1) != img).sum())} bytes differ")
    return bad


def quantiser_input(R, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, K, generator=g) * torch.exp2(torch.randint(-12, 12, (R, K // 32), generator=g).float()).repeat_interleave(32, dim=1)
    x.view(R, K // 32, 32)[torch.rand(R, K // 32, generator=g) < 0.1] = 0.0
    x[torch.rand(R, K, generator=g) < 4.0 / K] *= 64.0
    return x.to(dtype)


@pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "f32"))
@pytest.mark.parametrize("layout", (0, 1, 2))
def test_mx_quantize_codes_and_whole_image(dev, layout, dtype):
    bad = []
    for R in F8.QUANT_R:
        for K in F8.QUANT_K:
            bad += quantise_and_compare(quantiser_input(R, K, dtype, 100 * R + K), layout, f"layout {layout} R={R} K={K}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", (BF16, F32), ids=("bf16", "f32"))
@pytest.mark.parametrize("layout", (0, 1, 2))
def test_mx_quantize_constructed_blocks(dev, layout, dtype):
    """refs64_fp8.constructed_blocks in each of the four K-blocks of a 128-wide row in turn, random blocks beside them."""
    blocks = F8.constructed_blocks(dtype)
    bad = []
    for kb in range(4):
        x = quantiser_input(blocks.shape[0], 128, dtype, 7 + kb)
        x[:, 32 * kb:32 * kb + 32] = blocks
        bad += quantise_and_compare(x, layout, f"layout {layout} block {kb}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ norm -> MX in one pass
@pytest.mark.parametrize("d", F8.NORM_D)
@pytest.mark.parametrize("rms", (False, True), ids=("layernorm", "rmsnorm"))
def test_norm_mxq(dev, rms, d):
    from test_bytemovers_gpu import bar_of, check, family, wb
    bad = []
    worst = 0.0
    for rows, fam, want_y, want_rstd in F8.norm_cases(rms, d):
        what = f"{'rmsnorm' if rms else 'layernorm'} d={d} rows={rows} {fam} y={want_y} rstd={want_rstd}"
        x = family(fam, rows, d, BF16, 13)
        w, b = wb(d, BF16)
        b = None if rms else b
        ref, c32, ref_rstd, c32_rstd = F8.norm_ref(x, w, b, rms)
        bar = Bar.fp32_bar(ref, c32)
        qbuf = torch.full((rows + 2, d + 32), 0x55, device="cuda", dtype=U8)
        q, sc, y, rstd = ops.norm_mxq(x, w, b, eps=F8.NORM_EPS, want_y=want_y, want_rstd=want_rstd, q=qbuf[1:1 + rows, 16:16 + d])
        torch.cuda.synchronize()
        qh = q.cpu()
        e, pad = F8.read_image(sc, 0, rows, d)
        qbuf[1:1 + rows, 16:16 + d] = 0x55
        if int(pad.count_nonzero()) or int((qbuf != 0x55).sum()):
            bad.append(f"{what}: padded scale bytes not zero, or codes stored outside [rows, d] (ldq = d + 32)")
        blocks, over, ratio = F8.quant_errors(qh, e, ref, bar)
        worst = max(worst, ratio)
        if blocks or over:
            bad.append(f"{what}: {blocks} exponents outside the admissible set, {over} elements beyond step / 2 + bar (worst {ratio:.3f}x)")
        blk_m, el_m = F8.can_move(ref, bar)
        if F8.norm_exact(rms, fam):              # the result is the bf16 bias itself: nothing is exempt from equality, ties included
            blk_m, el_m = torch.zeros_like(blk_m), torch.zeros_like(el_m)
        rc, re = MX.quantize(ref.float())
        ne, nc = int(((e != re) & ~blk_m).sum()), int(((qh != rc) & ~el_m).sum())
        if ne or nc:
            bad.append(f"{what}: {ne} exponents and {nc} codes differ from the rule where the bar leaves no choice")
        if want_y:
            check(y, ref, bar_of(ref, c32, BF16), what + " y")
        if want_rstd:              # RMSNorm: the bar of test_rmsnorm_fwd; LayerNorm's optional rstd: the any-order derivation of bars.ln_rstd_bar
            check(rstd, ref_rstd, Bar.fp32_bar(ref_rstd, c32_rstd) if rms else Bar.ln_rstd_bar(x.double().cpu()) * ref_rstd, what + " rstd")
    assert not bad, "\n".join(bad)
    print(f"RATIO norm_mxq {'rmsnorm' if rms else 'layernorm'} d={d} {worst:.3f}")
