"""Kernel-level parity of the connector-training kernels against the float64 restatements of tests/refs64_connector.py: avllm_fuse_pool_bwd
(csrc/elementwise.hip) and avllm_gemm_wgrad (csrc/gemm_wgrad.hip), both dtypes.  Bars: tests/bars.py, "memory-bound kernels against float64"
-- 4 x the error of the same arithmetic in fp32 on the host, floored at 2 ulp, plus 2^-8 |ref| for a bf16 output; the weight gradient's outputs
are fp32 sums of exact products, the same rule.  Every case runs twice: neither kernel uses atomics, so the two results are the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64_connector as RC  # noqa: E402
import refs64_gemm as G  # noqa: E402
from avllm import ops  # noqa: E402

DT = {"f32": torch.float32, "bf16": torch.bfloat16}

# (Ta, Tv, P, L, S_out): equal / pool / interpolate / S_out == 1 on the two-input geometry; audio only and video only with P = 0 (pool and
# interpolate); Ta > L, whose rows t >= L must come out as exact zeros
GEOMS = [(9, 7, 3, 9, 12), (9, 7, 3, 9, 5), (9, 7, 3, 9, 20), (9, 7, 3, 9, 1), (9, 0, 0, 9, 4), (0, 7, 0, 7, 11), (12, 7, 2, 9, 8)]


def check(out, ref64, bar, what):
    o = out.detach().double().cpu()
    assert o.shape == ref64.shape, (what, o.shape, ref64.shape)
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite output"
    d = (o - ref64).abs()
    over = d - bar
    print(f"{what}: max |err| {float(d.max()):.3e}, bar {float(torch.as_tensor(bar).max()):.3e}")
    assert float(over.max()) <= 0.0, f"{what}: max |err| {float(d.max()):.3e} exceeds the bar by {float(over.max()):.3e}"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("D", [8, 4096])
@pytest.mark.parametrize("Ta,Tv,P,L,S", GEOMS)
def test_fuse_pool_bwd_vs_float64(dev, Ta, Tv, P, L, S, D, dt):
    dtype, B, fs = DT[dt], 2, 0.3
    g = torch.Generator().manual_seed(1000 * S + D + Ta)
    dx = torch.randn(B, S, D, generator=g).to(dtype)
    ra, rv = RC.fuse_pool_bwd(dx, Ta, Tv, P, L, fs)
    ca, cv = RC.fuse_pool_bwd(dx.float(), Ta, Tv, P, L, fs, dtype=torch.float32)
    da, dv = ops.fuse_pool_bwd(dx.to(dev), Ta, Tv, P, L, fs)
    da2, dv2 = ops.fuse_pool_bwd(dx.to(dev), Ta, Tv, P, L, fs)
    for nm, out, out2, ref, cpu in (("da", da, da2, ra, ca), ("dv", dv, dv2, rv, cv)):
        if ref is None:
            assert out is None
            continue
        bar = Bar.fp32_bar(ref, cpu)
        if dtype == torch.bfloat16:
            bar = Bar.bf16_bar(ref, bar)
        check(out, ref, bar, f"fuse_pool_bwd {nm} {dt} D={D} {(Ta, Tv, P, L, S)}")
        assert torch.equal(out, out2), f"{nm}: two launches differ"
    if Ta > L:
        assert float(da[:, L:].float().abs().max()) == 0.0
    # one output alone is the same values
    if Ta and Tv:
        only_a, none_v = ops.fuse_pool_bwd(dx.to(dev), Ta, Tv, P, L, fs, want_v=False)
        assert none_v is None and torch.equal(only_a, da)


WG = [(M, N, K) for M in (1, 63, 64, 65, 200) for (N, K) in ((64, 64), (128, 192))] + [(300, 4096, 768)]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,N,K", WG)
def test_gemm_wgrad_vs_float64(dev, M, N, K, dt):
    dtype, alpha = DT[dt], 0.37
    g = torch.Generator().manual_seed(M * 7 + N + K)
    dY = torch.randn(M, N, generator=g).to(dtype)
    X = torch.randn(M, K, generator=g).to(dtype)
    rW, rb = RC.gemm_wgrad(dY, X, alpha)
    cW, cb = RC.gemm_wgrad(dY.float(), X.float(), alpha, dtype=torch.float32)
    dW, db = ops.gemm_wgrad(dY.to(dev), X.to(dev), alpha)
    dW2, db2 = ops.gemm_wgrad(dY.to(dev), X.to(dev), alpha)
    assert dW.dtype == torch.float32 and db.dtype == torch.float32
    check(dW, rW, Bar.fp32_bar(rW, cW), f"gemm_wgrad dW {dt} M={M} N={N} K={K}")
    check(db, rb, Bar.fp32_bar(rb, cb), f"gemm_wgrad db {dt} M={M} N={N}")
    assert torch.equal(dW, dW2) and torch.equal(db, db2), "two launches differ"
    # dW as a view (row 1, column 8 on, ldw = K + 16 > K) of a NaN buffer: the same bits, and everything outside the view is still NaN
    buf = torch.full((N + 4, K + 16), float("nan"), device=dev, dtype=torch.float32)
    ops.gemm_wgrad(dY.to(dev), X.to(dev), alpha, dW=buf[1:1 + N, 8:8 + K])
    canary, over, _ = G.verify(buf, 1, 8, torch.arange(N, device=dev), K, dW.double(), 0.0)
    assert canary == 0 and over == 0, f"gemm_wgrad {dt} M={M} N={N} K={K} into a view: {over} differ, {canary} canaries overwritten"
    # the zero-bar families of tests/refs64_gemm.py (small integers: every partial sum is an integer the fp32 accumulator holds, alpha = 0.5 keeps
    # it a half-integer): ANY difference is an error, and with the one-hot dY of "locate" a wrong value names its tile
    for fam in G.ZERO_BAR:
        p, q, _ = G.family_tn(fam, M, N, K)
        ref = G.gemm_tn(p, q, alpha=0.5)
        rb0 = 0.5 * p.double().sum(0)
        assert torch.equal(ref.out, ref.out.float().double()) and torch.equal(rb0, rb0.float().double())
        buf = torch.full((N + 4, K + 16), float("nan"), device=dev, dtype=torch.float32)
        _, db0 = ops.gemm_wgrad(p.to(dtype).to(dev), q.to(dtype).to(dev), 0.5, dW=buf[1:1 + N, 8:8 + K])
        canary, over, _ = G.verify(buf, 1, 8, torch.arange(N, device=dev), K, ref.out.to(dev), 0.0)
        assert canary == 0 and over == 0, f"gemm_wgrad {fam} {dt} M={M} N={N} K={K}: {over} wrong, {canary} canaries overwritten"
        assert torch.equal(db0.double().cpu(), rb0), f"gemm_wgrad db {fam} {dt} M={M} N={N}"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gemm_wgrad_strided_rows_and_no_bias(dev, dt):
    """Row strides larger than the widths (a slice of a wider buffer), db left out."""
    dtype = DT[dt]
    g = torch.Generator().manual_seed(5)
    big_y, big_x = torch.randn(70, 96, generator=g).to(dtype).to(dev), torch.randn(70, 64, generator=g).to(dtype).to(dev)
    dY, X = big_y[:, 16:80], big_x[:, 8:48]
    rW, _ = RC.gemm_wgrad(dY.cpu(), X.cpu())
    cW, _ = RC.gemm_wgrad(dY.cpu().float(), X.cpu().float(), dtype=torch.float32)
    dW, db = ops.gemm_wgrad(dY, X, want_db=False)
    assert db is None
    check(dW, rW, Bar.fp32_bar(rW, cW), f"gemm_wgrad strided {dt}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("N,K", [(12, 64), (64, 20)])
def test_gemm_wgrad_refuses_unsupported_width(dev, N, K, dt):
    dY = torch.zeros(16, N, device=dev, dtype=DT[dt])
    X = torch.zeros(16, K, device=dev, dtype=DT[dt])
    with pytest.raises(ValueError, match="gemm_wgrad"):
        ops.gemm_wgrad(dY, X)


def test_grad_sumsq_multi_fixed_order(dev):
    """One norm over several buffers (clip_grad_norm_ over connector and LoRA gradients together): float64 reference, fp32_bar from the host's
    fp32 sum, and the same bits twice."""
    g = torch.Generator().manual_seed(3)
    bufs = [torch.randn(n, generator=g) for n in (33024, 7, 1 << 20)]
    ref = sum((b.double() ** 2).sum() for b in bufs).reshape(1)
    cpu = sum((b ** 2).sum() for b in bufs).reshape(1)
    parts = torch.zeros(1024, device=dev)
    outs = []
    for _ in range(2):
        out = torch.full((1,), 123.0, device=dev)
        ops.grad_sumsq_multi([b.to(dev) for b in bufs], out, parts)
        outs.append(out)
    check(outs[0], ref, Bar.fp32_bar(ref, cpu), "grad_sumsq_multi")
    assert torch.equal(outs[0], outs[1])


def test_adamw_multi_decay_groups_and_one_guard(dev):
    """Segments with their own weight decay under ONE guard: equal to avllm_adamw_step per segment on a good step; with zero gradients only the
    decayed segment moves (biases see no decay); a non-finite guard leaves every segment untouched and is counted -- and the step count taken
    back -- exactly once, however many segments the launch carries."""
    import ctypes
    from avllm import lib as L
    g = torch.Generator().manual_seed(9)
    mk = lambda n: [torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    segs = [mk(5000), mk(64), mk(333)]
    wds = [0.01, 0.0, 0.01]
    ref = [[t.clone() for t in s] for s in segs]
    sumsq = torch.tensor([sum(float((s[1].double() ** 2).sum()) for s in segs)], device=dev, dtype=torch.float32)
    guard, skipped = torch.ones(1, device=dev), torch.zeros(1, device=dev)
    ops.adamw_step_multi([(s[0], s[1], s[2], s[3], wd) for s, wd in zip(segs, wds)], 1e-3, 3, sumsq=sumsq, max_norm=0.5, guard=guard, skipped=skipped)
    for s, wd in zip(ref, wds):
        ops.adamw_step(s[0], s[1], s[2], s[3], 1e-3, 3, sumsq=sumsq, max_norm=0.5, wd=wd, guard=guard, skipped=skipped)
    # the same expressions compiled twice: a product may be fused into the following add in one kernel and not in the other, one rounding per
    # operation of the update chain (8 of them) at the most
    for s, r in zip(segs, ref):
        for a, b in zip(s, r):
            assert float((a - b).abs().max()) <= 8 * Bar.U32 * float(b.abs().max()) + 1e-30
    assert float(skipped) == 0.0
    # zero gradients: p * (1 - lr * wd) on the decayed segments, nothing on the other
    zs = [[s[0].clone(), torch.zeros_like(s[1]), torch.zeros_like(s[2]), torch.zeros_like(s[3])] for s in segs]
    ops.adamw_step_multi([(s[0], s[1], s[2], s[3], wd) for s, wd in zip(zs, wds)], 1e-3, 1)
    assert torch.equal(zs[1][0], segs[1][0]) and not torch.equal(zs[0][0], segs[0][0])
    assert torch.equal(zs[0][0], segs[0][0] * (1.0 - torch.tensor(1e-3, dtype=torch.float32) * torch.tensor(0.01, dtype=torch.float32)).to(dev))
    # non-finite guard with a device step state
    state = torch.zeros(ctypes.sizeof(L.StepState), dtype=torch.uint8, device=dev)
    ops.step_advance(state, 1e-3, 10)
    ops.step_advance(state, 1e-3, 10)
    keep = [[t.clone() for t in s] for s in segs]
    guard.fill_(float("nan"))
    ops.adamw_step_multi([(s[0], s[1], s[2], s[3], wd) for s, wd in zip(segs, wds)], 0.0, 0, sumsq=sumsq, max_norm=0.5, guard=guard, skipped=skipped,
                         state=state)
    assert all(torch.equal(a, b) for s, r in zip(segs, keep) for a, b in zip(s, r))
    st = state.cpu().numpy()
    assert float(skipped) == 1.0 and int(st.view("uint32")[0]) == 1 and float(st.view("float32")[5]) == 1.0


def test_gemm_wgrad_refuses_misaligned_operands(dev):
    """A column slice that starts 8 bytes into a row passes every width rule and would make misaligned 16-byte loads: refused."""
    big = torch.zeros(16, 80, device=dev, dtype=torch.bfloat16)
    ok = torch.zeros(16, 64, device=dev, dtype=torch.bfloat16)
    for dY, X in ((big[:, 4:68], ok), (ok, big[:, 4:68])):
        with pytest.raises(ValueError, match="16-byte aligned"):
            ops.gemm_wgrad(dY, X)


def test_grad_sumsq_multi_small_buffer_first(dev):
    """A large buffer behind a small one and behind another large one (the connector buffer precedes the LoRA buffer): same value as the
    float64 sum, whatever share of the partial slots each buffer gets."""
    g = torch.Generator().manual_seed(4)
    bufs = [torch.randn(n, generator=g) for n in (3 << 20, 5, 5 << 20)]
    ref = sum((b.double() ** 2).sum() for b in bufs).reshape(1)
    cpu = sum((b ** 2).sum() for b in bufs).reshape(1)
    out, parts = torch.zeros(1, device=dev), torch.zeros(1024, device=dev)
    ops.grad_sumsq_multi([b.to(dev) for b in bufs], out, parts)
    check(out, ref, Bar.fp32_bar(ref, cpu), "grad_sumsq_multi, three buffers")
