"""The GEMM kernels (csrc/gemm.hip, gemm_dp.hip, gemm_tn.hip, gemm_tn_kernel of loss_optim.hip) against the float64 restatements of
tests/refs64_gemm.py, at every kernel av_gemm_plan can name, one row / column past each tile and every epilogue form the plan lets that kernel take.
Bars: tests/bars.py ("GEMM against float64"); none is taken from a kernel's output, the exact and locate families carry the bar 0, and
tests/test_gemm_refs_cpu.py shows on the host that the documented arithmetic stays under each while nine mutants do not.

Every call first asserts the kernel ops.gemm(..., plan=True) names.  C is a view (row 1, column 8 on) of a larger NaN buffer with ldc > N and spare
rows: afterwards everything outside the written set must still be NaN (with a remap that includes the row the remap skips).  The dropout mask is
the numpy restatement of common.h (refs64_gemm.keep), never another kernel.  Each case prints "RATIO kernel family o(bf16|f32) act worst"."""
import collections
import contextlib
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64_gemm as G  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
R0, C0 = 1, 8
RATIOS = collections.defaultdict(float)
ACT_NAME = {0: "none", 1: "gelu", 2: "quick_gelu", 3: "silu"}


def note(kernel, fam, out_bf16, act, ratio):
    key = (kernel, fam, "o(bf16)" if out_bf16 else "o(f32)", ACT_NAME[act])
    RATIOS[key] = max(RATIOS[key], ratio)


def report(kernels):
    for key in sorted(RATIOS):
        if key[0] in kernels:
            print("RATIO", *key, f"{RATIOS[key]:.3f}")


def dev_(t, dtype):
    return None if t is None else t.to(dtype).cuda()


def strided(t, dtype):
    """t [rows, cols] -> a column slice (offset 8, row stride cols + 24) of a NaN buffer on the GPU."""
    wide = torch.full((t.shape[0], t.shape[1] + 24), float("nan"), device="cuda", dtype=dtype)
    view = wide[:, 8:8 + t.shape[1]]
    view.copy_(t.to(dtype))
    return view


def variant_of(kernel):
    return L.knob("GEMM_VARIANT", G.VARIANT[kernel]) if G.VARIANT.get(kernel) else contextlib.nullcontext()


@functools.lru_cache(maxsize=8)
def operands(fam, M, N, K, K2, r_rows):
    return G.family(fam, M, N, K, K2, r_rows=r_rows)


def build_case(fam, M, N, K, K2, e, kind, f32_in=False, libm=None, a_drop=None, n_valid=0):
    """-> everything a launch and its check need, computed once and shared by the kernels that take the case."""
    r_rows = e.r_mod if e.r_mod else M
    d = operands(fam, M, N, K, K2, r_rows)
    if n_valid > 0:                                   # the caller's side of n_valid (include/avllm.h): rows [n_valid, 64) of B are zero
        d = dict(d, B=d["B"].clone())
        d["B"][n_valid:] = 0
    bias = d["bias"] if e.bias else None
    drop = (G.DROP_SEED, G.drop_p(fam)) if e.drop else None
    R = d["R"] if e.R else None
    if fam == "offset" and e.R and not e.r_mod:
        R = G.cancel_R(G.gemm(d["A"], d["B"], d["A2"], d["B2"], bias=bias, act=e.act, alpha=e.alpha, drop=drop).out, r_rows)
    ref = G.gemm(d["A"], d["B"], d["A2"], d["B2"], bias=bias, R=R, act=e.act, alpha=e.alpha, r_mod=e.r_mod, remap=e.remap, drop=drop, a_drop=a_drop,
                 n_valid=n_valid)
    out_bf16 = not (e.f32 or f32_in)
    if fam == "exact":
        assert G.exact_holds(ref) or not out_bf16
    bar = 0.0 if fam in G.ZERO_BAR else Bar.gemm_bar(ref, K + K2, kind, e.act, e.alpha, out_bf16, libm).cuda()
    dt = F32 if f32_in else BF16
    A = strided(d["A"], dt) if e.strided else dev_(d["A"], dt)
    return dict(A=A, B=dev_(d["B"], dt), A2=dev_(d["A2"], dt), B2=dev_(d["B2"], dt), bias=dev_(bias, dt), R=dev_(R, dt), drop=drop, ref=ref.out.cuda(),
                rows=ref.rows.cuda(), total_rows=int(ref.rows.max()) + 1 + R0 + 3, bar=bar, out_bf16=out_bf16, M=M, N=N, e=e, a_drop=a_drop, n_valid=n_valid)


def launch(c, kernel, what):
    """Plan, run into a fresh NaN buffer, verify; returns the failure text or None."""
    e, M, N = c["e"], c["M"], c["N"]
    buf = torch.full((c["total_rows"], (N + 3) // 4 * 4 + 16), float("nan"), device="cuda", dtype=BF16 if c["out_bf16"] else F32)
    out = buf[R0:R0 + c["total_rows"] - R0 - 3, C0:C0 + N]
    R = c["R"]
    if e.inplace:
        out[:M].copy_(R)
        R = out[:M]
    kw = dict(out=out, bias=c["bias"], R=R, A2=c["A2"], B2=c["B2"], act=e.act, alpha=e.alpha, out_f32=e.f32, r_mod=e.r_mod, remap=e.remap, M=M,
              drop=c["drop"], a_drop=c["a_drop"], n_valid=c["n_valid"])
    planned = ops.gemm(c["A"], c["B"], plan=True, **kw)
    assert planned == kernel, f"{what}: planned on {planned}, not {kernel}"
    ops.gemm(c["A"], c["B"], **kw)
    torch.cuda.synchronize()
    canary, over, ratio = G.verify(buf, R0, C0, c["rows"], N, c["ref"], c["bar"])
    if canary or over:
        return f"{what}: {over}/{M * N} beyond the bar (worst {ratio:.2f}x), {canary} canaries overwritten"
    return ratio


def run_all(cases):
    """cases: iterable of (kernel, fam, case dict, what, context).  Collects every failure of the parametrised case before asserting."""
    bad = []
    n = 0
    for kernel, fam, c, what, ctx in cases:
        with ctx:
            r = launch(c, kernel, what)
        n += 1
        if isinstance(r, str):
            bad.append(r)
        else:
            note(kernel, fam, c["out_bf16"], c["e"].act, r)
    assert not bad, f"{len(bad)}/{n} calls failed:\n" + "\n".join(bad[:40])
    return n


# ------------------------------------------------------------------------------------------------ the tiled kernels
def tiled_cases(M, N, K, K2):
    for fam in G.FAMILIES:
        for e in G.EPIS:
            if not G.epi_ok(fam, e):
                continue
            c = build_case(fam, M, N, K, K2, e, "mfma")
            for kernel in G.TILED:
                takes = G.accepts(kernel, M, N, K, K2, e)
                if not takes and kernel != "128":
                    with variant_of(kernel), (L.knob("NARROW_EPILOGUE", 1) if e.narrow else contextlib.nullcontext()):
                        assert ops.gemm(c["A"], c["B"], plan=True, A2=c["A2"], B2=c["B2"], bias=c["bias"], R=c["R"], act=e.act, alpha=e.alpha, out_f32=e.f32,
                                        r_mod=e.r_mod, remap=e.remap, drop=c["drop"]) == "128", (kernel, e.name)       # a forced variant that cannot take the call
                    continue
                ctx = contextlib.ExitStack()
                ctx.enter_context(_deferred(variant_of, kernel))
                if e.narrow:
                    ctx.enter_context(_deferred(L.knob, "NARROW_EPILOGUE", 1))
                yield kernel, fam, c, f"{kernel} {M}x{N}x{K}+{K2} {fam} {e.name}", ctx


class _deferred:
    """A context manager built on entry (the knob is read and set when the launch happens, not when the case list is built)."""

    def __init__(self, fn, *a):
        self.fn, self.a = fn, a

    def __enter__(self):
        self.cm = self.fn(*self.a)
        return self.cm.__enter__()

    def __exit__(self, *exc):
        return self.cm.__exit__(*exc)


@pytest.mark.parametrize("K,K2", G.TILE_K, ids=lambda v: str(v))
@pytest.mark.parametrize("M,N", G.TILE_MN, ids=lambda v: str(v))
def test_tiled_kernels(dev, M, N, K, K2):
    n = run_all(tiled_cases(M, N, K, K2))
    print(f"CALLS {n}")
    report(G.TILED)


# ------------------------------------------------------------------------------------------------ persistent kernels, several tiles per workgroup
@functools.lru_cache(maxsize=4)
def big_exact(fam, M, N, K):
    """Full-size zero-bar reference: fp32 host products of integers (every partial sum is an integer the fp32 format holds)."""
    d = G.family(fam, M, N, K)
    return d, (d["A"] @ d["B"].t())


@pytest.mark.parametrize("gw", (0, 3))
@pytest.mark.parametrize("K", G.PERSIST_K)
@pytest.mark.parametrize("kernel", ("HP16", "WP4", "DP"))
def test_persistent_walk(dev, kernel, K, gw):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tm, tn, th, tw = (34, 16, 256, 128) if kernel == "DP" else (17, 16, 256, 256)
    M, N = tm * th - 3, tn * tw - 8
    per_cu = 2 if kernel == "DP" else 1                       # the 256 x 128 kernel keeps two workgroups per CU
    assert tm * tn > cus * per_cu, f"{tm * tn} tiles do not exceed the {cus * per_cu} resident workgroups: nothing walks"
    bad = []
    with L.knob("GEMM_VARIANT", G.VARIANT[kernel]), L.knob("GEMM_GW", gw):
        for fam in G.ZERO_BAR:
            d, acc = big_exact(fam, M, N, K)
            for name in ("plain", "bias_R"):
                bias, R = (d["bias"], d["R"]) if name == "bias_R" else (None, None)
                want = acc if bias is None else acc + bias[None, :] + R
                assert torch.equal(want, want.to(BF16).to(F32))
                buf = torch.full((M + R0 + 3, N + 16), float("nan"), device="cuda", dtype=BF16)
                out = buf[R0:R0 + M, C0:C0 + N]
                kw = dict(out=out, bias=dev_(bias, BF16), R=dev_(R, BF16))
                A, B = dev_(d["A"], BF16), dev_(d["B"], BF16)
                assert ops.gemm(A, B, plan=True, **kw) == kernel
                ops.gemm(A, B, **kw)
                torch.cuda.synchronize()
                canary, over, _ = G.verify(buf, R0, C0, torch.arange(M, device="cuda"), N, want.double().cuda(), 0.0)
                if canary or over:
                    wrong = (out.float().cpu() != want).nonzero()
                    bad.append(f"{kernel} {fam} {name} K={K} gw={gw}: {over} wrong, {canary} canaries; first at {wrong[:4].tolist()}")
        rows = G.sample_rows(M)
        for fam in ("randn", "offset", "heavy"):
            d = G.family(fam, M, N, K)
            for e in (G.EPIS[0], G.EPIS[3], G.EPIS[7]):
                bias, R = (d["bias"] if e.bias else None), (d["R"] if e.R else None)
                ref = G.gemm(d["A"][rows], d["B"], bias=bias, R=None if R is None else R[rows], act=e.act)
                bar = Bar.gemm_bar(ref, K, "mfma", e.act, 1.0, True, libm=(kernel == "HP16"))
                buf = torch.full((M + R0 + 3, N + 16), float("nan"), device="cuda", dtype=BF16)
                out = buf[R0:R0 + M, C0:C0 + N]
                kw = dict(out=out, bias=dev_(bias, BF16), R=dev_(R, BF16), act=e.act)
                A, B = dev_(d["A"], BF16), dev_(d["B"], BF16)
                assert ops.gemm(A, B, plan=True, **kw) == kernel
                ops.gemm(A, B, **kw)
                torch.cuda.synchronize()
                got = buf.clone()
                keep = torch.ones(buf.shape[0], dtype=torch.bool, device="cuda")
                keep[rows.cuda() + R0] = False
                got[keep, C0:C0 + N] = float("nan")                     # rows not sampled: only their being written at all is checked
                assert bool(torch.isfinite(out.float()).all()), f"{kernel} {fam} {e.name}: unwritten output"
                canary, over, ratio = G.verify(got, R0, C0, rows.cuda(), N, ref.out.cuda(), bar.cuda())
                canary += int((~torch.isnan(buf[:, :C0].float())).sum() + (~torch.isnan(buf[:, C0 + N:].float())).sum() + (~torch.isnan(buf[:R0].float())).sum()
                              + (~torch.isnan(buf[R0 + M:].float())).sum())
                if canary or over:
                    bad.append(f"{kernel} {fam} {e.name} K={K} gw={gw}: {over} beyond the bar ({ratio:.2f}x), {canary} canaries")
                else:
                    note(kernel + "-walk", fam, True, e.act, ratio)
    assert not bad, "\n".join(bad)
    report((kernel + "-walk",))


# ------------------------------------------------------------------------------------------------ SMALLM, SKINNY64, F32
@pytest.mark.parametrize("K", G.SMALLM_K)
@pytest.mark.parametrize("M", G.SMALLM_M)
def test_smallm(dev, M, K):
    def cases():
        for N in G.SMALLM_N:
            for K2 in G.SMALLM_K2:
                for fam in G.FAMILIES:
                    for e in G.SMALLM_EPIS:
                        if G.epi_ok(fam, e):
                            yield "SMALLM", fam, build_case(fam, M, N, K, K2, e, "split8", libm=True), f"SMALLM {M}x{N}x{K}+{K2} {fam} {e.name}", contextlib.nullcontext()
    run_all(cases())
    report(("SMALLM",))


@pytest.mark.parametrize("K", G.SKINNY_K)
@pytest.mark.parametrize("M", G.SKINNY_M)
def test_skinny64(dev, M, K):
    """n_valid: rows [n_valid, 64) of B are zero, as include/avllm.h asks of the caller; the columns from 16 ceil(n_valid / 16) on are exactly 0 and
    WRITTEN (the reference holds 0 there with sum_abs 0, so the bar is the denormal floor, and a column left alone would still be NaN).  Three
    16-column groups (n_valid = 33) run the four-group body: the last group's zeros then come from B's zero rows.  a_drop: host keep on index m K + k, the scaled A re-rounded to bf16."""
    def cases():
        for nv in G.SKINNY_NV:
            for fam in G.FAMILIES:
                for a_drop in ((G.DROP_SEED, G.drop_p(fam)), None):
                    if a_drop is None and M < 256:
                        continue                                # the plan gives M < 256 to this kernel only with the fused mask
                    for e in (G.Epi("alpha", alpha=0.5), G.Epi("f32", f32=True, alpha=2.0)):
                        c = build_case(fam, M, 64, K, 0, e, "split8", a_drop=a_drop, n_valid=nv)
                        yield "SKINNY64", fam, c, f"SKINNY64 {M}x64x{K} nv={nv} {fam} {e.name} a_drop={a_drop is not None}", contextlib.nullcontext()
    run_all(cases())
    report(("SKINNY64",))


@pytest.mark.parametrize("K,K2", [(k, k2) for k in G.F32_K for k2 in G.F32_K2], ids=lambda v: str(v))
@pytest.mark.parametrize("M,N", G.F32_MN, ids=lambda v: str(v))
def test_f32(dev, M, N, K, K2):
    def cases():
        for fam in G.FAMILIES:
            for e in G.F32_EPIS:
                if G.epi_ok(fam, e):
                    yield "F32", fam, build_case(fam, M, N, K, K2, e, "f32", f32_in=True, libm=True), f"F32 {M}x{N}x{K}+{K2} {fam} {e.name}", contextlib.nullcontext()
    run_all(cases())
    report(("F32",))


# ------------------------------------------------------------------------------------------------ gemm_tn / gemm_tn_drop
def tn_case(fam, M, I, J, p_is_big, dt, drop, what):
    """p_is_big: P [M, I] is the wide operand (out [I, J]); else the operands swap (out [J, I], the transposed store).  The narrow operand is a
    16-column slice of a wider buffer whose columns J.. are NaN (the MFMA path reads 16 columns and must store J); both operands are strided."""
    big, small, o = G.family_tn(fam, M, I, J)
    o = o if p_is_big else o.t().contiguous()
    P, Q = (big, small) if p_is_big else (small, big)
    pi, qj = (I, J) if p_is_big else (J, I)
    alpha = 0.5
    ref = G.gemm_tn(P, Q, alpha=alpha, drop=drop, out=o)
    mfma = dt == BF16 and I % 128 == 0 and J <= 16
    bar = 0.0 if fam in G.ZERO_BAR else Bar.gemm_tn_bar(ref, M, alpha, o.double(), mfma).cuda()
    bigd = strided(big, dt)
    sm = torch.full((M, 40), float("nan"), device="cuda", dtype=dt)
    sm[:, 8:8 + J].copy_(small.to(dt))
    smalld = sm[:, 8:8 + max(J, 16)]
    Pd, Qd = (bigd, smalld) if p_is_big else (smalld, bigd)
    buf = torch.full((pi + R0 + 3, (qj + 3) // 4 * 4 + 16), float("nan"), device="cuda", dtype=F32)
    out = buf[R0:R0 + pi, C0:C0 + qj]
    out.copy_(o)
    ops.gemm_tn(Pd, Qd, out, I=pi, J=qj, alpha=alpha, drop=drop)
    torch.cuda.synchronize()
    canary, over, ratio = G.verify(buf, R0, C0, torch.arange(pi, device="cuda"), qj, ref.out.cuda(), bar)
    if canary or over:
        return f"{what}: {over}/{pi * qj} beyond the bar (worst {ratio:.2f}x), {canary} canaries overwritten"
    note("TN_MFMA" if mfma else "TN_SCALAR", fam, False, 0, ratio)
    return None


@pytest.mark.parametrize("M", G.TN_M)
def test_gemm_tn_mfma(dev, M):
    bad = []
    for I in G.TN_I:
        for J in G.TN_J:
            for p_is_big in (True, False):
                for fam in G.FAMILIES:
                    for drop in (None, (G.DROP_SEED, G.drop_p(fam))):
                        what = f"gemm_tn{'_drop' if drop else ''} M={M} I={I} J={J} {'[I,J]' if p_is_big else '[J,I]'} {fam}"
                        r = tn_case(fam, M, I, J, p_is_big, BF16, drop, what)
                        if r:
                            bad.append(r)
    assert not bad, f"{len(bad)} failed:\n" + "\n".join(bad[:40])
    report(("TN_MFMA",))


@pytest.mark.parametrize("dt", (BF16, F32), ids=("bf16", "f32"))
@pytest.mark.parametrize("I,J", ((272, 8), (128, 17), (272, 17)), ids=lambda v: str(v))
def test_gemm_tn_scalar(dev, I, J, dt):
    bad = []
    for M in (1, 65, 257, 1000):
        for p_is_big in (True, False):
            for fam in G.FAMILIES:
                r = tn_case(fam, M, I, J, p_is_big, dt, None, f"gemm_tn scalar M={M} I={I} J={J} {'[I,J]' if p_is_big else '[J,I]'} {fam}")
                if r:
                    bad.append(r)
    assert not bad, f"{len(bad)} failed:\n" + "\n".join(bad[:40])
    report(("TN_SCALAR",))


# ------------------------------------------------------------------------------------------------ refusals stay refusals
def test_refusals(dev):
    refused = (ValueError, L.AvllmError)
    A = torch.zeros(300, 96, device="cuda", dtype=BF16)
    with pytest.raises(refused):
        ops.gemm(A, torch.zeros(64, 96, device="cuda", dtype=BF16))                       # K % 64 != 0
    A = torch.zeros(300, 256, device="cuda", dtype=BF16)
    with pytest.raises(refused):
        ops.gemm(A, torch.zeros(128, 256, device="cuda", dtype=BF16), a_drop=(1, 0.05))   # a_drop with N != 64
    with pytest.raises(refused):
        ops.gemm(torch.zeros(300, 512, device="cuda", dtype=BF16)[:, :256], torch.zeros(64, 256, device="cuda", dtype=BF16), a_drop=(1, 0.05))      # lda != K
    with pytest.raises(refused):                                                          # K2 = 32: the entry check wants whole 64-column K tiles in both segments
        ops.gemm(torch.zeros(4, 256, device="cuda", dtype=BF16), torch.zeros(16, 256, device="cuda", dtype=BF16),
                 A2=torch.zeros(4, 32, device="cuda", dtype=BF16), B2=torch.zeros(16, 32, device="cuda", dtype=BF16))
    out = torch.zeros(272, 8, device="cuda", dtype=F32)
    with pytest.raises(refused):
        ops.gemm_tn(torch.zeros(64, 272, device="cuda", dtype=BF16), torch.zeros(64, 16, device="cuda", dtype=BF16), out, J=8, drop=(1, 0.05))      # drop off the MFMA path
    assert bool((out == 0).all())
