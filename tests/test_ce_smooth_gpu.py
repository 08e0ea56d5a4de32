"""Kernel-level parity of the smoothed cross entropy (csrc/loss_optim.hip: ce_smooth_fwd_kernel / ce_smooth_bwd_kernel through ops.ce_smooth_fwd /
ops.ce_smooth_bwd) against the float64 restatement of tests/refs64_loss.py, in the manner of test_bytemovers_gpu.test_cross_entropy: the same
inputs (logit scales 1 and 30, the late +80 spike, the five label patterns, a padded buffer with a sentinel), bars built in refs64_loss from
bars.py, never from a kernel's output.

Shapes: V = 5 (tail only), 8 (one bf16 vector, two fp32), 1000 (whole vectors), 1001 (a tail of 1), 2049 (bf16: second trip of the 256-thread
loop holds only the tail; fp32: third), 32003 (many trips + a tail of 3), each at B*T = 80, and V = 1001 at 2 x 2048 rows (more rows than CUs
x occupancy).  Pairs trimmed as test_cross_entropy trims them: the label patterns other than "all" run at scale 30 and B*T = 80 with
(0.1, 1e-4); "all" runs all four (eps, z)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64_loss as RL  # noqa: E402
from avllm import ops  # noqa: E402
from test_bytemovers_gpu import check  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}
SHAPES = [(5, 8, 2, 40), (8, 8, 2, 40), (1000, 1000, 2, 40), (1001, 1008, 2, 40), (2049, 2056, 2, 40), (32003, 32008, 2, 40), (1001, 1008, 2, 2048)]
OPTIONS = [(0.1, 0.0), (0.0, 1e-2), (0.1, 1e-4), (0.9, 1.0)]
GS = 0.37


def cases():
    out = []
    for dn, dt in DT.items():
        for V, ld, B, T in SHAPES:
            for sc in (1, 30):
                for pat in (RL.PATTERNS if (B * T == 80 and sc == 30) else ["all"]):
                    for eps, z in (OPTIONS if pat == "all" else [(0.1, 1e-4)]):
                        out.append(pytest.param(dt, V, ld, B, T, sc, pat, eps, z, id=f"{dn}-V{V}ld{ld}-B{B}T{T}-scale{sc}-{pat}-eps{eps}-z{z}"))
    return out


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def inputs(dtype, V, ld, B, T, scale, pat):
    buf, _ = RL.ce_logits(B, T, V, ld, scale, dtype)
    buf = buf.cuda()
    return buf, buf[:, :, :V], RL.ce_labels(pat, B, T, V).cuda()


@pytest.mark.parametrize("dtype,V,ld,B,T,scale,pat,eps,z", cases())
def test_ce_smooth(dev, dtype, V, ld, B, T, scale, pat, eps, z):
    buf, logits, labels = inputs(dtype, V, ld, B, T, scale, pat)
    ref_lse, ref_sum, ref_cnt, ref_terms, ref_g = RL.smooth_cross_entropy(logits, labels, eps, z, grad_scale=GS)
    row_lse, acc, terms = ops.ce_smooth_fwd(logits, labels, eps, z)
    lb = RL.lse_bar(logits, ref_lse)
    check(row_lse, ref_lse, lb, "ce_smooth_fwd row_lse")
    assert float(acc[1]) == ref_cnt, (float(acc[1]), ref_cnt)
    if ref_cnt == 0:
        assert float(acc[0]) == 0.0 and float(terms.abs().max()) == 0.0
    else:
        term_bars, loss_bar = RL.sum_bars(logits, labels, eps, z)
        for name, got, ref, bar in zip(("nll", "u", "q"), terms.tolist(), ref_terms.tolist(), term_bars):
            print(f"ce_smooth_fwd terms[{name}]: err {abs(got - ref):.3e}, bar {bar:.3e}, sum {ref:.6e}")
            assert abs(got - ref) <= bar, (name, got, ref, bar)
        print(f"ce_smooth_fwd loss_sum: err {abs(float(acc[0]) - float(ref_sum)):.3e}, bar {loss_bar:.3e}, sum {float(ref_sum):.6e}")
        assert abs(float(acc[0]) - float(ref_sum)) <= loss_bar
    dl = ops.ce_smooth_bwd(logits, labels, row_lse, acc, eps, z, grad_scale=GS)
    assert dl.stride() == logits.stride()
    if ref_cnt == 0:
        assert float(dl.float().abs().max()) == 0.0 and not bool(torch.isnan(dl.float()).any())
    else:
        bar = RL.grad_bar(logits, labels, eps, z, GS, ref_lse, ref_cnt, lb)
        check(dl, ref_g, bar + Bar.BF16_OUT_REL * ref_g.abs() if dtype == BF16 else bar, "ce_smooth_bwd")
    # in place == out of place, padding untouched, a second launch gives the same bits
    inplace = buf.clone()
    lv = inplace[:, :, :V]
    out = ops.ce_smooth_bwd(lv, labels, row_lse, acc, eps, z, grad_scale=GS, out=lv)
    assert out.data_ptr() == lv.data_ptr()
    assert torch.equal(bits(lv), bits(dl)), "in place != out of place"
    assert bool((inplace[:, :, V:] == 7.0).all()) and bool((buf[:, :, V:] == 7.0).all()), "padding columns written"
    row_lse2, acc2, _ = ops.ce_smooth_fwd(logits, labels, eps, z)
    dl2 = ops.ce_smooth_bwd(logits, labels, row_lse2, acc2, eps, z, grad_scale=GS)
    assert torch.equal(bits(row_lse2), bits(row_lse)) and torch.equal(bits(dl2), bits(dl)), "two launches differ"


@pytest.mark.parametrize("pat", ["all", "beyond_vocab", "none"])
@pytest.mark.parametrize("V,ld", [(5, 8), (1001, 1008), (2049, 2056), (32003, 32008)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_both_off_gives_the_plain_kernels_bits(dev, dtype, V, ld, pat):
    """(0, 0): row_lse, count and dlogits are those of ops.ce_fwd / ops.ce_bwd bit for bit; loss_sum and terms[0] up to the atomics' order."""
    buf, logits, labels = inputs(dtype, V, ld, 2, 40, 30, pat)
    lse0, acc0 = ops.ce_fwd(logits, labels)
    dl0 = ops.ce_bwd(logits, labels, lse0, acc0, grad_scale=GS)
    lse1, acc1, terms = ops.ce_smooth_fwd(logits, labels, 0.0, 0.0)
    dl1 = ops.ce_smooth_bwd(logits, labels, lse1, acc1, 0.0, 0.0, grad_scale=GS)
    assert torch.equal(bits(lse0), bits(lse1)) and float(acc0[1]) == float(acc1[1])
    assert torch.equal(bits(dl0), bits(dl1))
    tol = Bar.atomic_sum_term(max(1.0, float(acc0[1])), float(acc0[0]))
    assert abs(float(acc0[0]) - float(acc1[0])) <= tol and abs(float(acc0[0]) - float(terms[0])) <= tol


def test_options_out_of_range_are_refused_by_name(dev):
    logits = torch.zeros(2, 4, 16, device=dev)
    labels = torch.zeros(2, 4, dtype=torch.int64, device=dev)
    row_lse, acc = ops.ce_fwd(logits, labels)
    for eps, z, name in ((1.0, 0.0, "label_smoothing=1.0"), (-0.1, 0.0, "label_smoothing=-0.1"), (float("nan"), 0.0, "label_smoothing=nan"),
                         (0.1, -1e-4, "z_loss=-0.0001"), (0.1, float("nan"), "z_loss=nan"), (0.1, float("inf"), "z_loss=inf")):
        with pytest.raises(ValueError, match=name):
            ops.ce_smooth_fwd(logits, labels, eps, z)
        with pytest.raises(ValueError, match=name):
            ops.ce_smooth_bwd(logits, labels, row_lse, acc, eps, z)
    # the C entry points refuse them too (AV_ERR_ARG), whatever the caller checked
    from avllm import lib as L
    for eps, z in ((1.0, 0.0), (-0.1, 0.0), (0.0, -1.0), (float("nan"), 0.0), (0.0, float("nan"))):
        rc = L.load().avllm_ce_smooth_fwd(L.ptr(logits), 16, L.ptr(labels), 2, 4, 16, eps, z, L.ptr(row_lse), L.ptr(acc), L.ptr(acc) + 4, None,
                                          L.dt_of(logits), L.stream_ptr())
        assert rc == 1, (eps, z, rc)
        rc = L.load().avllm_ce_smooth_bwd(L.ptr(logits), 16, L.ptr(labels), L.ptr(row_lse), L.ptr(acc) + 4, 1.0, eps, z, L.ptr(logits), 2, 4, 16,
                                          L.dt_of(logits), L.stream_ptr())
        assert rc == 1, (eps, z, rc)


def test_views_and_strides_are_checked_as_for_the_plain_pair(dev):
    logits = torch.zeros(2, 4, 16, device=dev)
    labels = torch.zeros(2, 4, dtype=torch.int64, device=dev)
    row_lse, acc, _ = ops.ce_smooth_fwd(logits, labels, 0.1, 0.0)
    with pytest.raises(ValueError, match="out must have"):
        ops.ce_smooth_bwd(logits[:, :, :9], labels, row_lse, acc, 0.1, 0.0, out=torch.empty(2, 4, 9, device=dev))
    with pytest.raises(ValueError, match="rows of one stride"):
        ops.ce_smooth_bwd(torch.zeros(2, 4, 9, device=dev), labels, row_lse, acc, 0.1, 0.0)
    with pytest.raises(ValueError, match="rows of one stride"):
        ops.ce_smooth_fwd(torch.zeros(2, 4, 9, device=dev), labels, 0.1, 0.0)
