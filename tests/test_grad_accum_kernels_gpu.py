"""The kernels of gradient accumulation against float64 and against the entries they extend: avllm_gemm_wgrad_acc (csrc/gemm_wgrad.hip),
avllm_adamw_step_dev / avllm_adamw_step_multi_dev, avllm_step_advance_micro and avllm_window_add (csrc/loss_optim.hip).
Bars: tests/bars.py fp32_bar -- 4 x the error of the same arithmetic in fp32 on the host, floored at 2 ulp -- as tests/test_connector_kernels_gpu.py
holds avllm_gemm_wgrad to, evaluated on the host for dW0 + alpha * acc (the accumulating form's one extra rounding is inside it); the AdamW bars
are those of tests/test_bytemovers_gpu.py::test_adamw and test_connector_kernels_gpu.py::test_adamw_multi_decay_groups_and_one_guard."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64 as R  # noqa: E402
import refs64_connector as RC  # noqa: E402
import refs64_gemm as G  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402
from test_grad_accum_host_cpu import micro_seed  # noqa: E402  (the header's rule, restated once)

DT = {"f32": torch.float32, "bf16": torch.bfloat16}
M32 = 0xFFFFFFFF

# (M, N, K, pad): one cell; ragged in all three against the 128 x 128 x 64 and 64 x 64 x 32 tiles; exact tiles, two slabs plus 2 rows; ldw = K + 8
SHAPES = [(1, 8, 8, 0), (65, 136, 264, 0), (130, 128, 128, 0), (65, 136, 264, 8)]
SENTINEL = -12345.0


def check(out, ref64, bar, what):
    o = out.detach().double().cpu()
    assert o.shape == ref64.shape and bool(torch.isfinite(o).all()), what
    d = float((o - ref64).abs().max())
    print(f"{what}: max |err| {d:.3e}, bar {bar:.3e}")
    assert d <= bar, f"{what}: max |err| {d:.3e} exceeds the bar {bar:.3e}"


def padded(dW0, pad, dev):
    """dW0 as the leading K columns of an [N, K + pad] device buffer whose pad cells hold the sentinel."""
    N, K = dW0.shape
    buf = torch.full((N, K + pad), SENTINEL, dtype=torch.float32)
    buf[:, :K] = dW0
    buf = buf.to(dev)
    return buf, buf[:, :K]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,N,K,pad", SHAPES)
def test_wgrad_acc_vs_float64(dev, M, N, K, pad, dt):
    dtype, alpha = DT[dt], 0.37
    g = torch.Generator().manual_seed(M * 7 + N + K + pad)
    dY, X = torch.randn(M, N, generator=g).to(dtype), torch.randn(M, K, generator=g).to(dtype)
    rW, rb = RC.gemm_wgrad(dY, X, alpha)
    cW, cb = RC.gemm_wgrad(dY.float(), X.float(), alpha, dtype=torch.float32)
    W0 = torch.randn(N, K, generator=g) * float(rW.abs().max())               # a prior value of the product's size
    b0 = torch.randn(N, generator=g) * float(rb.abs().max())
    buf, view = padded(W0, pad, dev)
    db = b0.to(dev)
    ops.gemm_wgrad_acc(dY.to(dev), X.to(dev), view, db, alpha=alpha)
    check(view, W0.double() + rW, Bar.fp32_bar(W0.double() + rW, W0 + cW), f"wgrad_acc dW {dt} {(M, N, K, pad)}")
    check(db, b0.double() + rb, Bar.fp32_bar(b0.double() + rb, b0 + cb), f"wgrad_acc db {dt} {(M, N, K, pad)}")
    if pad:
        assert bool((buf[:, K:] == SENTINEL).all()), "cells past K were written"
    # the integer family: small-integer operands and prior value, every sum an integer fp32 holds -- any difference is an error
    p, q, o = G.family_tn("exact", M, N, K)
    ref = o.double() + 0.5 * (p.double().t() @ q.double())
    rb0 = o[:, 0].double() + 0.5 * p.double().sum(0)
    assert torch.equal(ref, ref.float().double())
    buf, view = padded(o, pad, dev)
    db = o[:, 0].clone().to(dev)
    ops.gemm_wgrad_acc(p.to(dtype).to(dev), q.to(dtype).to(dev), view, db, alpha=0.5)
    assert torch.equal(view.double().cpu(), ref) and torch.equal(db.double().cpu(), rb0), f"wgrad_acc exact {dt} {(M, N, K, pad)}"
    if pad:
        assert bool((buf[:, K:] == SENTINEL).all())


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("M,N,K,pad", SHAPES)
def test_wgrad_acc_bitwise(dev, M, N, K, pad, dt):
    dtype, alpha = DT[dt], 0.37
    g = torch.Generator().manual_seed(M + 3 * N + K + pad)
    dY, X = torch.randn(3 * M, N, generator=g).to(dtype).to(dev), torch.randn(3 * M, K, generator=g).to(dtype).to(dev)
    # onto zeros: the overwriting entry's bits
    W, b = ops.gemm_wgrad(dY[:M], X[:M], alpha)
    buf, view = padded(torch.zeros(N, K), pad, dev)
    db = torch.zeros(N, device=dev)
    ops.gemm_wgrad_acc(dY[:M], X[:M], view, db, alpha=alpha)
    assert torch.equal(view, W) and torch.equal(db, b), "onto zeros the accumulating form differs from avllm_gemm_wgrad"
    # two launches from one prior value: the same bits
    W0, b0 = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    outs = []
    for _ in range(2):
        buf, view = padded(W0, pad, dev)
        db = b0.to(dev)
        ops.gemm_wgrad_acc(dY[:M], X[:M], view, db, alpha=alpha)
        outs.append((view.clone(), db.clone()))
        assert bool((buf[:, K:] == SENTINEL).all()), "the sentinel past K was touched"
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # three chained launches == one launch on the row-concatenated operands, within the bar of the whole sum
    buf, view = padded(W0, pad, dev)
    db = b0.to(dev)
    for j in range(3):
        ops.gemm_wgrad_acc(dY[j * M:(j + 1) * M], X[j * M:(j + 1) * M], view, db, alpha=alpha)
    rW, rb = RC.gemm_wgrad(dY.cpu(), X.cpu(), alpha)
    cW, cb = RC.gemm_wgrad(dY.cpu().float(), X.cpu().float(), alpha, dtype=torch.float32)
    check(view, W0.double() + rW, Bar.fp32_bar(W0.double() + rW, W0 + cW), f"wgrad_acc chained dW {dt} {(M, N, K, pad)}")
    check(db, b0.double() + rb, Bar.fp32_bar(b0.double() + rb, b0 + cb), f"wgrad_acc chained db {dt} {(M, N, K, pad)}")
    buf1, view1 = padded(W0, pad, dev)
    db1 = b0.to(dev)
    ops.gemm_wgrad_acc(dY, X, view1, db1, alpha=alpha)
    check(view1, W0.double() + rW, Bar.fp32_bar(W0.double() + rW, W0 + cW), f"wgrad_acc one launch dW {dt} {(M, N, K, pad)}")


def test_wgrad_acc_refusals(dev):
    for N, K in ((12, 64), (64, 20)):
        with pytest.raises(ValueError, match="gemm_wgrad"):
            ops.gemm_wgrad_acc(torch.zeros(16, N, device=dev), torch.zeros(16, K, device=dev), torch.zeros(N, K, device=dev))


# ---------------------------------------------------------------------------------------------------------------- AdamW, device divisor
def new_state(dev, step=0, skipped=0.0, micro=0):
    st = L.StepState()
    st.step, st.skipped = step, skipped
    st.reserved[0] = micro
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).clone().to(dev)


def read_state(state):
    return L.StepState.from_buffer_copy(bytes(state.cpu().numpy().tobytes()))


@pytest.mark.parametrize("count", [1.0, 37.0, 0.0])
@pytest.mark.parametrize("max_norm", [0.5, 0.0])
def test_adamw_device_divisor_vs_float64(dev, count, max_norm):
    """20 steps against the float64 rule with prescale = 1 / count (0 at count 0), the bar of test_bytemovers_gpu.py::test_adamw."""
    n, lr0, wd = 5003, 3e-3, 0.01
    gen = lambda s: torch.Generator().manual_seed(s)
    pre = float(torch.tensor(1.0) / torch.tensor(count)) if count > 0 else 0.0          # the header's rule: the fp32 quotient
    p0 = torch.randn(n, generator=gen(71))
    p, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p32, m32, v32 = p0.clone(), torch.zeros(n), torch.zeros(n)
    parts, ss, div = torch.zeros(1024, device=dev), torch.zeros(1, device=dev), torch.tensor([count], device=dev)
    for s in range(1, 21):
        g = (torch.randn(n, generator=gen(1000 + s)) * (0.3 * max(count, 1.0))).to(dev)
        lr = R.schedule(s, lr0, 60)[0]
        ops.grad_sumsq(g, ss, partials=parts)
        ops.adamw_step(p, g, m, v, lr, s, sumsq=ss, max_norm=max_norm, wd=wd, grad_div=div)
        gc = g.cpu()
        coef = R.clip_coef(float((gc.double() ** 2).sum()), max_norm, pre)
        R.adamw_step(p64, gc.double(), m64, v64, lr, s, coef=coef, wd=wd)
        R.adamw_step(p32, gc, m32, v32, lr, s, coef=coef, wd=wd)
    for nm, a, r64, r32 in (("p", p, p64, p32), ("m", m, m64, m32), ("v", v, v64, v32)):
        check(a, r64, Bar.fp32_bar(r64, r32), f"adamw_dev {nm} count={count} max_norm={max_norm}")
    if count == 0.0:
        assert float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0          # zero gradient, step taken (decay only)
        assert not torch.equal(p.cpu(), p0)


def _segs(dev, seed=9):
    g = torch.Generator().manual_seed(seed)
    mk = lambda n: [torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    return [mk(5000), mk(64), mk(333)], [0.01, 0.0, 0.01]


@pytest.mark.parametrize("count", [1.0, 37.0, 0.0])
def test_adamw_multi_device_divisor(dev, count):
    """The multi form with a device divisor against avllm_adamw_step per segment at grad_prescale = 1 / count, by the bar of
    test_adamw_multi_decay_groups_and_one_guard (8 roundings of the update chain); count = 1 against the existing multi entry: the same bits."""
    segs, wds = _segs(dev)
    ref = [[t.clone() for t in s] for s in segs]
    sumsq = torch.tensor([sum(float((s[1].double() ** 2).sum()) for s in segs)], device=dev, dtype=torch.float32)
    div = torch.tensor([count], device=dev)
    pre = float(torch.tensor(1.0) / torch.tensor(count)) if count > 0 else 0.0          # the fp32 quotient the kernel forms
    ops.adamw_step_multi([(s[0], s[1], s[2], s[3], wd) for s, wd in zip(segs, wds)], 1e-3, 3, sumsq=sumsq, max_norm=0.5, grad_div=div)
    for s, wd in zip(ref, wds):
        ops.adamw_step(s[0], s[1], s[2], s[3], 1e-3, 3, sumsq=sumsq, max_norm=0.5, wd=wd, prescale=pre)
    for s, r in zip(segs, ref):
        for a, b in zip(s, r):
            assert float((a - b).abs().max()) <= 8 * Bar.U32 * float(b.abs().max()) + 1e-30
    if count == 1.0:
        segs2, _ = _segs(dev)
        ops.adamw_step_multi([(s[0], s[1], s[2], s[3], wd) for s, wd in zip(segs2, wds)], 1e-3, 3, sumsq=sumsq, max_norm=0.5, prescale=1.0)
        assert all(torch.equal(a, b) for s, r in zip(segs, segs2) for a, b in zip(s, r))


def test_adamw_device_divisor_one_is_the_existing_entry(dev):
    n = 4099
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(n, generator=g), torch.randn(n, generator=g), torch.rand(n, generator=g), torch.rand(n, generator=g)]
    ss, div = torch.tensor([float((base[1].double() ** 2).sum())], device=dev), torch.ones(1, device=dev)
    a, b = [t.to(dev) for t in base], [t.to(dev) for t in base]
    ops.adamw_step(a[0], a[1], a[2], a[3], 1e-3, 4, sumsq=ss, max_norm=0.5, prescale=1.0)
    ops.adamw_step(b[0], b[1], b[2], b[3], 1e-3, 4, sumsq=ss, max_norm=0.5, grad_div=div)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("bad", ["sumsq_inf", "guard_nan"])
def test_adamw_device_divisor_skips_once(dev, bad, multi):
    segs, wds = _segs(dev, 11)
    keep = [[t.clone() for t in s] for s in segs]
    ss = torch.tensor([float("inf") if bad == "sumsq_inf" else 1.0], device=dev)
    guard = torch.tensor([float("nan") if bad == "guard_nan" else 2.0], device=dev)
    skipped, div = torch.zeros(1, device=dev), torch.tensor([37.0], device=dev)
    state = new_state(dev, step=3, micro=2)
    if multi:
        ops.adamw_step_multi([(s[0], s[1], s[2], s[3], wd) for s, wd in zip(segs, wds)], 0.0, 0, sumsq=ss, max_norm=0.5, guard=guard, skipped=skipped,
                             state=state, grad_div=div)
    else:
        s = segs[0]
        ops.adamw_step(s[0], s[1], s[2], s[3], 0.0, 0, sumsq=ss, max_norm=0.5, guard=guard, skipped=skipped, state=state, grad_div=div)
    assert all(torch.equal(a, b) for s, r in zip(segs, keep) for a, b in zip(s, r))
    st = read_state(state)
    assert float(skipped) == 1.0 and st.step == 2 and st.skipped == 1.0 and st.reserved[0] == 0


# ---------------------------------------------------------------------------------------------------------------- the micro-step advance
def test_micro_advance_two_windows(dev):
    base, total, warm, rank = 1e-3, 50, 2, 1
    ref = new_state(dev)
    state = new_state(dev)
    p, g, m, v = (torch.ones(8, device=dev) for _ in range(4))
    ss, div, skipped = torch.ones(1, device=dev), torch.ones(1, device=dev), torch.zeros(1, device=dev)
    for window, guard_val in enumerate((2.0, float("nan"), 2.0)):          # taken, skipped, taken
        ops.step_advance(ref, base, total, warm, rank=rank)
        want = read_state(ref)
        seeds = []
        for micro in range(3):
            ops.step_advance_micro(state, base, total, warm, rank=rank)
            st = read_state(state)
            assert (st.step, st.lr, st.bc1, st.bc2_sqrt) == (want.step, want.lr, want.bc1, want.bc2_sqrt), (window, micro)
            assert st.reserved[0] == micro + 1
            assert st.dropout_seed == micro_seed(st.step, int(st.skipped), micro, rank=rank), (window, micro)
            seeds.append(st.dropout_seed)
        assert seeds[0] == want.dropout_seed and len(set(seeds)) == 3          # micro-step 0 keeps avllm_step_advance's seed
        guard = torch.tensor([guard_val], device=dev)
        for s in (state, ref):
            ops.adamw_step(p.clone(), g, m.clone(), v.clone(), 0.0, 0, sumsq=ss, guard=guard, skipped=skipped, state=s, grad_div=div)
        st, want = read_state(state), read_state(ref)
        assert st.reserved[0] == 0 and st.step == want.step and st.skipped == want.skipped
        assert st.step == (1 if window < 2 else 2) and st.skipped == (0.0 if window == 0 else 1.0)


def test_window_add_fixed_order(dev):
    window = torch.tensor([7.0, 7.0], device=dev)
    state = new_state(dev, micro=1)                        # right after the first advance of a window: overwrite
    ops.window_add(window, torch.tensor([1.5, 3.0], device=dev), state)
    assert window.tolist() == [1.5, 3.0]
    state = new_state(dev, micro=2)
    ops.window_add(window, torch.tensor([0.25, 5.0], device=dev), state)
    assert window.tolist() == [1.75, 8.0]
    ops.window_add(window, torch.tensor([float("nan"), 0.0], device=dev), state)
    assert window[0].isnan() and float(window[1]) == 8.0
    assert ctypes.sizeof(L.StepState) == 32
