"""avllm_lora_merge (csrc/lora_merge.hip) against float64 (tests/refs64_merge.py) under the bar of tests/bars_merge.py: every shape below at ranks
1, 4, 16 and 64, row strides K and K + 8, scales 2.0 and -0.5, f32 and bf16 storage, always as a slice that starts at row 5 of a taller matrix
whose other rows -- and the 8 padding columns when the stride exceeds K -- hold a sentinel that must survive.  Families: exact (every result
representable: any difference is an error), locate (one-hot operands: one element moves, by exactly the expected amount), gauss, and offset
(W = -scale B.A + noise: the result is a cancellation, which holds the kernel to its single rounding).  Two launches give equal bytes, scale 0
returns W bit for bit, and every refusal of the header leaves the buffer alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import refs64_merge as M  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402
from bars_merge import merge_bar  # noqa: E402

SHAPES = [(1, 8), (3, 136), (64, 128), (130, 264), (256, 512)]      # one element group; odd rows, two strips; one tile; ragged tiles; 4 x 4 tiles
RANKS = (1, 4, 16, 64)
SCALES = (2.0, -0.5)
GUARD, SENTINEL = 5, -3.0        # rows before and after the slice; exactly representable in both storage types


def _operands(family, N, K, r, scale, dtype, g):
    """(W, A, B) on the CPU: W in the storage type, the masters fp32."""
    if family == "exact":            # |u| <= r <= 64, |scale u| <= 128 in halves, |W| <= 8: at most 8 significant bits, a bf16 value
        A = torch.randint(-1, 2, (r, K), generator=g).float()
        B = torch.randint(-1, 2, (N, r), generator=g).float()
        W = torch.randint(-8, 9, (N, K), generator=g).float()
    elif family == "locate":
        A, B = torch.zeros(r, K), torch.zeros(N, r)
        j, k, n = (int(torch.randint(0, m, (1,), generator=g)) for m in (r, K, N))
        A[j, k], B[n, j] = 4.0, -0.75
        W = torch.randint(-8, 9, (N, K), generator=g).float()
    else:
        A, B = torch.randn(r, K, generator=g), torch.randn(N, r, generator=g)
        W = torch.randn(N, K, generator=g)
        if family == "offset":
            W = (-scale * (B.double() @ A.double()) + 1e-3 * W.double()).float()
    return W.to(dtype), A, B


def _framed(W, ldw, dev):
    """W copied into rows GUARD .. GUARD + N of a sentinel-filled [N + 2 GUARD, ldw] device matrix -> (the matrix, the [N, K] view)."""
    N, K = W.shape
    buf = torch.full((N + 2 * GUARD, ldw), SENTINEL, dtype=W.dtype, device=dev)
    view = buf[GUARD:GUARD + N, :K]
    view.copy_(W)
    return buf, view


def _frame_untouched(buf, N, K):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[GUARD + N:] == SENTINEL).all() and (buf[:, K:] == SENTINEL).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("family", ["exact", "locate", "gauss", "offset"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_merge_against_float64(dev, N, K, family, dtype):
    g = torch.Generator().manual_seed(1000 * N + K)
    worst = 0.0
    for r in RANKS:
        for ldw in (K, K + 8):
            for scale in SCALES:
                W, A, B = _operands(family, N, K, r, scale, dtype, g)
                ref, u, sum_abs = M.merge64(W, A, B, scale)
                buf, view = _framed(W, ldw, dev)
                Ad, Bd = A.to(dev), B.to(dev)
                out = ops.lora_merge_(view, Ad, Bd, scale)
                assert out is view and _frame_untouched(buf, N, K), (r, ldw, scale)
                got = view.cpu()
                if family in ("exact", "locate"):
                    assert torch.equal(got.double(), ref), (r, ldw, scale)
                    if family == "locate":
                        moved = got != W
                        assert int(moved.sum()) == 1 and float((got.double() - W.double())[moved]) == scale * 4.0 * -0.75
                        assert torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)[~moved],
                                           W.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)[~moved])
                else:
                    ratio = (got.double() - ref).abs() / merge_bar(ref, u, sum_abs, r, scale, dtype == torch.bfloat16)
                    worst = max(worst, float(ratio.max()))
                    assert float(ratio.max()) <= 1.0, (r, ldw, scale, float(ratio.max()))
                # no atomics, one thread per element: a second launch on equal inputs writes equal bytes
                buf2, view2 = _framed(W, ldw, dev)
                ops.lora_merge_(view2, Ad, Bd, scale)
                assert torch.equal(buf2, buf)
    print(f"RATIO lora_merge {family} {'bf16' if dtype == torch.bfloat16 else 'f32'} N={N} K={K}: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_scale_zero_returns_w_bit_for_bit(dev, dtype):
    g = torch.Generator().manual_seed(7)
    W, A, B = _operands("gauss", 130, 264, 16, 0.0, dtype, g)
    W[3, 5] = -0.0
    buf, view = _framed(W, 272, dev)
    before = buf.clone()
    ops.lora_merge_(view, A.to(dev), B.to(dev), 0.0)
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(buf.view(bits), before.view(bits))


def test_refusals_leave_the_buffer_alone(dev):
    lib = L.load()
    N, K, r = 16, 32, 4
    for dtype in (torch.float32, torch.bfloat16):
        W = torch.full((N, K + 8), 1.5, dtype=dtype, device=dev)
        before = W.clone()
        A, B = torch.ones(r, K, device=dev), torch.ones(N, r, device=dev)
        dt = L.dt_of(W)

        def raw(w=L.ptr(W), ldw=K + 8, n=N, k=K, a=L.ptr(A), b=L.ptr(B), rank=r, dtype_id=dt):
            L.check(lib.avllm_lora_merge(w, ldw, n, k, a, b, rank, 2.0, dtype_id, L.stream_ptr()))

        es = W.element_size()
        for bad in (dict(w=None), dict(a=None), dict(b=None), dict(rank=0), dict(rank=-1), dict(rank=L.LORA_PAD + 1), dict(n=0), dict(n=-3),
                    dict(k=K - 4), dict(k=0), dict(ldw=K + 4), dict(ldw=K - 8), dict(w=L.ptr(W) + es), dict(w=L.ptr(W) + 8),
                    dict(dtype_id=2), dict(dtype_id=-1)):
            with pytest.raises(ValueError, match="lora_merge"):
                raw(**bad)
        # the tensor-level wrapper: shapes and dtypes that do not match, before the library is asked
        for w_, a_, b_ in ((W[:, :K], A[:, :K - 8].contiguous(), B), (W[:, :K], A, B[:N - 1].contiguous()), (W[:, :K], A[:r - 1].contiguous(), B),
                           (W[:, :K], A.to(torch.bfloat16), B), (W[:, :K].to(torch.float16), A, B), (W[:, :K].t(), B.t().contiguous(), A.t().contiguous()),
                           (W[:, :K], A.t().contiguous().t(), B)):
            with pytest.raises(ValueError, match="lora_merge"):
                ops.lora_merge_(w_, a_, b_, 2.0)
        torch.cuda.synchronize()
        assert torch.equal(W, before)
