"""Kernel-level checks of the per-clip modality kernels (csrc/modality.hip) against tests/refs64_modality.py: avllm_fuse_pool_rows and its
adjoint against float64 under the bars of test_connector_kernels_gpu.py::test_fuse_pool_bwd_vs_float64 (tests/bars.py: 4 x the error of the
same arithmetic in fp32 on the host, floored at 2 ulp, plus 2^-8 |ref| for a bf16 output), twice with equal bits; bit identity with
avllm_fuse_pool / avllm_fuse_pool_bwd under uniform modes; row independence; unused streams are not read; the draw against its restatement;
the refusals."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64_modality as RM  # noqa: E402
from avllm import ops  # noqa: E402
from test_connector_kernels_gpu import DT, check  # noqa: E402

# (Ta, Tv, P, L, S_out): identity / pool / interpolate / S_out == 1, and Ta > L
GEOMS = [(9, 7, 3, 9, 12), (9, 7, 3, 9, 5), (9, 7, 3, 9, 20), (9, 7, 3, 9, 1), (12, 7, 2, 9, 8)]
# one vector per row, a width that is no multiple of 8 (the bf16 adjoint takes its 4-wide form), one that is no power of two, the model width
# (more than one trip of a block's column loop)
WIDTHS = [8, 20, 136, 4096]
FS = 0.3


def inputs(Ta, Tv, P, S, D, dtype, B=3):
    g = torch.Generator().manual_seed(1000 * S + D + Ta)
    mk = lambda *shape: torch.randn(*shape, generator=g).to(dtype)
    return mk(B, Ta, D), mk(B, Tv, D), mk(B, P, D), mk(B, S, D)


def modes_dev(modes, dev):
    return torch.tensor(modes, dtype=torch.int32, device=dev)


def bar_for(ref, cpu, dtype):
    bar = Bar.fp32_bar(ref, cpu)
    return Bar.bf16_bar(ref, bar) if dtype == torch.bfloat16 else bar


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("Ta,Tv,P,L,S", GEOMS)
def test_rows_forward_and_adjoint_vs_float64(dev, Ta, Tv, P, L, S, D, dt):
    dtype, modes = DT[dt], [0, 1, 2]
    a, v, pe, dx = inputs(Ta, Tv, P, S, D, dtype)
    md = modes_dev(modes, dev)
    what = f"{dt} D={D} {(Ta, Tv, P, L, S)}"
    ref = RM.fuse_pool_rows(a, v, pe, modes, L, S, FS)
    cpu = RM.fuse_pool_rows(a.float(), v.float(), pe.float(), modes, L, S, FS, dtype=torch.float32)
    out = ops.fuse_pool_rows(a.to(dev), v.to(dev), pe.to(dev), md, L, S, FS, D, 3)
    out2 = ops.fuse_pool_rows(a.to(dev), v.to(dev), pe.to(dev), md, L, S, FS, D, 3)
    check(out, ref, bar_for(ref, cpu, dtype), "fuse_pool_rows " + what)
    assert torch.equal(out, out2), "two launches differ"
    ra, rv = RM.fuse_pool_rows_bwd(dx, modes, Ta, Tv, P, L, FS)
    ca, cv = RM.fuse_pool_rows_bwd(dx.float(), modes, Ta, Tv, P, L, FS, dtype=torch.float32)
    da, dv = ops.fuse_pool_rows_bwd(dx.to(dev), md, Ta, Tv, P, L, FS)
    da2, dv2 = ops.fuse_pool_rows_bwd(dx.to(dev), md, Ta, Tv, P, L, FS)
    for nm, o, o2, r, c in (("da", da, da2, ra, ca), ("dv", dv, dv2, rv, cv)):
        check(o, r, bar_for(r, c, dtype), f"fuse_pool_rows_bwd {nm} " + what)
        assert torch.equal(o, o2), f"{nm}: two launches differ"
    assert float(dv[1].float().abs().max()) == 0.0 and float(da[2].float().abs().max()) == 0.0
    if Ta > L:
        assert float(da[:, L:].float().abs().max()) == 0.0


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("Ta,Tv,P,L,S", GEOMS)
def test_uniform_modes_are_the_existing_kernels_bit_for_bit(dev, Ta, Tv, P, L, S, D, dt):
    """All 0 / all 1 / all 2 against avllm_fuse_pool and avllm_fuse_pool_bwd in their two-input and one-input forms at the same L; the mixed
    launch's row b is the uniform launch's row b; NaN in a stream a row does not use changes nothing."""
    dtype, B = DT[dt], 3
    a, v, pe, dx = (t.to(dev) for t in inputs(Ta, Tv, P, S, D, dtype))
    uniform = {}
    for m, (fa, fv, bTa, bTv) in {0: (a, v, Ta, Tv), 1: (a, None, Ta, 0), 2: (None, v, 0, Tv)}.items():
        md = modes_dev([m] * B, dev)
        out = ops.fuse_pool_rows(a, v, pe, md, L, S, FS, D, B)
        assert torch.equal(out, ops.fuse_pool(fa, fv, pe, L, S, FS, D, B)), f"forward, modes all {m}"
        da, dv = ops.fuse_pool_rows_bwd(dx, md, Ta, Tv, P, L, FS)
        ea, ev = ops.fuse_pool_bwd(dx, bTa, bTv, P, L, FS)
        for nm, got, want in (("da", da, ea), ("dv", dv, ev)):
            if want is None:
                assert float(got.float().abs().max()) == 0.0 and not bool(torch.signbit(got.float()).any()), f"{nm}, modes all {m}: not exact zeros"
            else:
                assert torch.equal(got, want), f"{nm}, modes all {m}"
        uniform[m] = (out, da, dv)
    modes = [0, 1, 2]
    md = modes_dev(modes, dev)
    out = ops.fuse_pool_rows(a, v, pe, md, L, S, FS, D, B)
    da, dv = ops.fuse_pool_rows_bwd(dx, md, Ta, Tv, P, L, FS)
    for b, m in enumerate(modes):
        for nm, got, want in zip(("out", "da", "dv"), (out, da, dv), uniform[m]):
            assert torch.equal(got[b], want[b]), f"{nm} row {b} (mode {m}) depends on the other rows' modes"
    na, nv = a.clone(), v.clone()
    na[2], nv[1] = float("nan"), float("nan")
    poisoned = ops.fuse_pool_rows(na, nv, pe, md, L, S, FS, D, B)
    assert bool(torch.isfinite(poisoned.float()).all()) and torch.equal(poisoned, out)
    # any other mode value reads as 0
    assert torch.equal(ops.fuse_pool_rows(a, v, pe, modes_dev([3, -1, 7], dev), L, S, FS, D, B), uniform[0][0])


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("B", [1, 16, 33])
def test_draw_is_the_restatement(dev, B, given):
    mode_in = [(b * 7 + 1) % 4 for b in range(B)] if given else None            # 0..3: 1 and 2 survive, 0 and 3 are drawn
    mi = modes_dev(mode_in, dev) if given else None
    for seed in (0, 12345, 0xDEADBEEF):
        for pa, pv in ((0.3, 0.3), (0.5, 0.5), (0.05, 0.0)):
            want = RM.draw(B, pa, pv, seed, mode_in)
            assert ops.modality_draw(B, pa, pv, seed=seed, mode_in=mi, device=dev).tolist() == want, (seed, pa, pv)
            w = (seed - 77) & 0xFFFFFFFF                                        # the device word and the by-value seed add up to `seed` mod 2^32
            word = torch.tensor([w if w < 1 << 31 else w - (1 << 32)], dtype=torch.int32, device=dev)
            out = torch.full((B,), -5, dtype=torch.int32, device=dev)
            got = ops.modality_draw(B, pa, pv, seed=77, seed_dev=word, mode_in=mi, out=out)
            assert got.data_ptr() == out.data_ptr() and got.tolist() == want, ("seed_dev", seed, pa, pv)
    if given:                                                                   # in place: mode_out aliases mode_in
        buf = mi.clone()
        ops.modality_draw(B, 0.3, 0.3, seed=5, mode_in=buf, out=buf)
        assert buf.tolist() == RM.draw(B, 0.3, 0.3, 5, mode_in)


def test_refusals(dev):
    a, v = torch.zeros(2, 4, 8, device=dev), torch.zeros(2, 3, 8, device=dev)
    md = modes_dev([0, 1], dev)
    with pytest.raises(ValueError, match="both inputs"):
        ops.fuse_pool_rows(a, None, None, md, 4, 4, FS, 8, 2)
    with pytest.raises(ValueError, match="both inputs"):
        ops.fuse_pool_rows(None, v, None, md, 4, 4, FS, 8, 2)
    with pytest.raises(ValueError, match="both inputs"):
        ops.fuse_pool_rows_bwd(torch.zeros(2, 4, 8, device=dev), md, 4, 0, 0, 4, FS)
    with pytest.raises(ValueError, match="fuse_pool_rows"):                      # D % 4
        ops.fuse_pool_rows(torch.zeros(2, 4, 6, device=dev), torch.zeros(2, 3, 6, device=dev), None, md, 4, 4, FS, 6, 2)
    with pytest.raises(ValueError, match="fuse_pool_rows_bwd"):
        ops.fuse_pool_rows_bwd(torch.zeros(2, 4, 6, device=dev), md, 4, 3, 0, 4, FS)
    with pytest.raises(ValueError, match="mode must be"):
        ops.fuse_pool_rows(a, v, None, md.long(), 4, 4, FS, 8, 2)
    with pytest.raises(ValueError, match="mode must be"):
        ops.fuse_pool_rows(a, v, None, modes_dev([0, 1, 2], dev), 4, 4, FS, 8, 2)
    with pytest.raises(ValueError, match="modality_draw"):                       # B <= 0
        ops.modality_draw(0, 0.3, 0.3, device=dev)
    with pytest.raises(ValueError, match="modality_draw"):
        ops.modality_draw(4, 0.7, 0.7, device=dev)
    # the C entry itself refuses a NULL input and B <= 0 (callers that bypass ops.py)
    from avllm import lib as L
    out = torch.zeros(2, 4, 8, device=dev)
    lib = L.load()
    for args in ((None, 4, L.ptr(v), 3, None, 0, L.ptr(md), L.ptr(out), 2, 4, 4, 8, FS, L.F32, L.stream_ptr()),
                 (L.ptr(a), 4, L.ptr(v), 3, None, 0, None, L.ptr(out), 2, 4, 4, 8, FS, L.F32, L.stream_ptr()),
                 (L.ptr(a), 4, L.ptr(v), 3, None, 0, L.ptr(md), L.ptr(out), 0, 4, 4, 8, FS, L.F32, L.stream_ptr())):
        with pytest.raises(ValueError, match="fuse_pool_rows"):
            L.check(lib.avllm_fuse_pool_rows(*args))
    with pytest.raises(ValueError, match="modality_draw"):
        L.check(lib.avllm_modality_draw(None, L.ptr(md), 0, 0.3, 0.3, 0, None, L.stream_ptr()))
