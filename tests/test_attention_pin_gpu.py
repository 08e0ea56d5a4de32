"""The attention kernels (csrc/attention.hip, attention_bwd.hip, attention_ref.hip) against the float64 restatements of tests/refs64_attention.py,
at every form av_attention_fwd / av_attention_bwd can select (named in each test id; every call first asserts that ops.attention_fwd / _bwd
(plan=True) names it) and at the tile edges of each.  Bars: tests/bars.py
("attention against float64"); none is taken from a kernel's output, and tests/test_attention_refs_cpu.py shows on the host that the documented
arithmetic stays under each while one unmasked / dropped / shifted key, a wrong kv head, a missing delta or query row does not.

Every call is made the guarded way: q, k and v are column slices of wider buffers whose other columns are NaN (row strides that are not the packed
width), outputs are views into buffers with a guard row and guard columns of a sentinel that must be untouched afterwards.  Families (randn, flat,
sharp, sharp_last, range, offset, count) are looped inside a case; each prints its worst error / bar ratio ("RATIO form tensor value")."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64_attention as A  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402

SENTINEL = 777.0
PAD = 8                      # guard / NaN columns on each side: slices stay 16-byte aligned, strides multiples of 8


def nan_wide(x, dtype, extra_rows=0):
    """x [rows, cols] (CPU) -> (wide NaN buffer on the GPU, view of x inside it)."""
    rows, cols = x.shape
    wide = torch.full((rows + extra_rows, cols + 2 * PAD), float("nan"), device="cuda", dtype=dtype)
    view = wide[:rows, PAD:PAD + cols]
    view.copy_(x.to(dtype))
    return wide, view


def guarded(rows, cols, dtype):
    buf = torch.full((rows + 1, cols + 2 * PAD), SENTINEL, device="cuda", dtype=dtype)
    return buf, buf[:rows, PAD:PAD + cols]


def guard_intact(buf, rows, cols, what):
    assert bool((buf[rows:] == SENTINEL).all()) and bool((buf[:, :PAD] == SENTINEL).all()) and bool((buf[:, PAD + cols:] == SENTINEL).all()), \
        f"{what}: wrote outside its output"


def knob_of(g):
    return L.knob("ATTN_SHORT", 0) if g.knob else contextlib.nullcontext()


def check(out, ref64, bar, what, tag):
    o = out.detach().double().cpu()
    assert o.shape == ref64.shape, (what, o.shape, ref64.shape)
    assert bool(torch.isfinite(o).all()), f"{what}: non-finite output"
    err = (o - ref64).abs()
    bar_t = bar if torch.is_tensor(bar) else torch.full_like(err, float(bar))
    worst = float((err / bar_t.clamp_min(1e-300)).max())
    print(f"RATIO {tag} {worst:.3f}   ({what}: max err {float(err.max()):.3e})")
    over = err > bar_t
    assert not bool(over.any()), f"{what}: {int(over.sum())}/{err.numel()} beyond the bar, worst {worst:.2f}x (max err {float(err.max()):.3e})"


def run_fwd(g, c, k_cpu=None, v_cpu=None):
    dt = c.storage
    d = g.H * g.hd
    _, qv = nan_wide(c.q, dt)
    _, kv = nan_wide(c.k if k_cpu is None else k_cpu, dt)
    _, vv = nan_wide(c.v if v_cpu is None else v_cpu, dt)
    obuf, ov = guarded(g.B * g.Tq, d, dt)
    kw = dict(impl=g.impl, kv_heads=g.Hkv, Tk=g.Tk, k=kv, v=vv, out=ov)
    with knob_of(g):
        planned = ops.attention_fwd(qv, g.B, g.Tq, g.H, g.hd, g.causal, plan=True, **kw)
        assert planned == A.kernel_of(g), f"{A.geo_id(g)}: planned on {planned}"
        o, lse = ops.attention_fwd(qv, g.B, g.Tq, g.H, g.hd, g.causal, **kw)
    torch.cuda.synchronize()
    guard_intact(obuf, g.B * g.Tq, d, "attention_fwd")
    return o, lse


@pytest.mark.parametrize("g", A.GEOMETRIES, ids=A.geo_id)
def test_forward(dev, g):
    for fam in A.FAMILIES:
        c = A.case(g, fam)
        o, lse = run_fwd(g, c)
        what = f"{A.geo_id(g)} {fam}"
        check(o, c.o64, c.bar_o, f"{what} o", f"{g.form}-{g.dt} o")
        check(lse, c.lse64, c.bar_lse, f"{what} lse", f"{g.form}-{g.dt} lse")
        if fam == "count":                                   # exp(lse) is the number of keys the query saw
            seen = torch.exp(lse.double().cpu()).round().long()
            assert bool((seen == c.n[None, None, :]).all()), f"{what}: keys seen {seen[0, 0].tolist()} != {c.n.tolist()}"


TQTK = [g for g in A.GEOMETRIES if g.Tq != g.Tk and (g.Tq, g.Tk) in ((33, 130), (50, 197), (150, 200))]


@pytest.mark.parametrize("g", TQTK, ids=A.geo_id)
def test_forward_next_item_never_read(dev, g):
    """Tq != Tk: item b's keys are rows [b Tk, (b + 1) Tk).  With the K / V rows of every later item NaN, item 0's output must not change by a bit."""
    c = A.case(g, "randn")
    o0, l0 = run_fwd(g, c)
    k, v = c.k.clone(), c.v.clone()
    k[g.Tk:], v[g.Tk:] = float("nan"), float("nan")
    o1, l1 = run_fwd(g, c, k, v)
    assert torch.equal(o0[:g.Tq], o1[:g.Tq]) and torch.equal(l0[0], l1[0])
    assert bool(torch.isnan(o1[g.Tq:].float()).all())           # and the later items did read their own rows


def run_bwd(g, c, rope_tab=None, impl=None):
    """Forward + backward on the fused [q | k | v] rows, a column slice of a NaN buffer -> (dq, dk, dv) views of the guarded output."""
    dt = c.storage
    d, dkv = g.H * g.hd, g.Hkv * g.hd
    impl = g.impl if impl is None else impl
    _, qkv = nan_wide(torch.cat([c.bq, c.bk, c.bv], 1), dt)
    dout = c.bdout.to(dt).cuda()
    gbuf, gv = guarded(g.B * g.Tq, d + 2 * dkv, dt)
    # the backward has no short form: those lengths run on its 64-key-tile kernels
    want = "ref" if impl else "mfma64x4" if A.kernel_of(g).startswith("short") else A.kernel_of(g)
    with knob_of(g):
        o, lse = ops.attention_fwd(qkv, g.B, g.Tq, g.H, g.hd, g.causal, impl=impl, kv_heads=g.Hkv)
        kw = dict(impl=impl, kv_heads=g.Hkv, rope_tab=rope_tab, out=gv)
        planned = ops.attention_bwd(qkv, o, dout, lse, g.B, g.Tq, g.H, g.hd, g.causal, plan=True, **kw)
        assert planned == want, f"{A.geo_id(g)}: backward planned on {planned}, not {want}"
        ops.attention_bwd(qkv, o, dout, lse, g.B, g.Tq, g.H, g.hd, g.causal, **kw)
    torch.cuda.synchronize()
    guard_intact(gbuf, g.B * g.Tq, d + 2 * dkv, "attention_bwd")
    return gv[:, :d], gv[:, d:d + dkv], gv[:, d + dkv:]


def check_bwd(g, c, got, what):
    for name, out, ref, bar, rl2 in (("dq", got[0], c.dq64, c.bar_dq, c.rel_l2_dq), ("dk", got[1], c.dk64, c.bar_dk, c.rel_l2_dk),
                                     ("dv", got[2], c.dv64, c.bar_dv, c.rel_l2_dv)):
        check(out, ref, bar, f"{what} {name}", f"{g.form}-{g.dt} {name}")
        o64 = out.double().cpu()
        # every head against its own bar (dq: query heads; dk, dv: kv heads), in every family: the per-head check the sharp families keep where
        # the relative-L2 bar does not apply
        for h, (cols, hbar) in enumerate(zip(A.head_cols(g, name), getattr(c, "hbar_" + name))):
            e = float((o64[:, cols] - ref[:, cols]).abs().max())
            print(f"RATIO {g.form}-{g.dt} {name}-head {e / hbar:.3f}")
            assert e <= hbar, f"{what} {name} head {h}: max err {e:.3e} > {hbar:.3e} ({e / hbar:.2f}x)"
        if rl2 is not None and float(ref.abs().max()) > 0:
            for h, cols in enumerate(A.head_cols(g, name) if name != "dq" else [slice(None)]):   # dk and dv: every kv head on its own
                e = Bar.rel_l2(o64[:, cols], ref[:, cols])
                print(f"RATIO {g.form}-{g.dt} {name}-rel_l2 {e / rl2:.3f}")
                assert e <= rl2, f"{what} {name} head {h}: relative L2 {e:.3e} > {rl2:.3e}"


@pytest.mark.parametrize("g", [g for g in A.GEOMETRIES if A.has_bwd(g)], ids=A.geo_id)
def test_backward(dev, g):
    for fam in A.FAMILIES:
        c = A.case(g, fam)
        got = run_bwd(g, c)
        what = f"{A.geo_id(g)} {fam}"
        check_bwd(g, c, got, what)
        if fam == "count":
            for name, out, ref, eb in (("dq", got[0], c.dq64, c.ebar_dq), ("dk", got[1], c.dk64, c.ebar_dk), ("dv", got[2], c.dv64, c.ebar_dv)):
                check(out, ref, eb, f"{what} {name} elementwise", f"{g.form}-{g.dt} count-{name}")


ROPE_GEO = [A._g("rope-bwd-mfma%dx4" % hd, 70, hd, True, "mfma", H=4, Hkv=2) for hd in (64, 128)]


@pytest.mark.parametrize("pos0", [0, 5])
@pytest.mark.parametrize("g", ROPE_GEO, ids=A.geo_id)
def test_backward_fused_inverse_rope(dev, g, pos0):
    """The form the engine runs in every bf16 train step: the inverse rotary fused into dq | dk.  Against attn_bwd64 with the rotary tail (the table
    is an input: both sides read the fp32 values avllm_rope_table wrote), and against the unfused sequence attention_bwd -> rope_tab_(inverse).
    Unfused, the rotation reads a pair (a, b) that was already rounded to bf16 (2^-8 (|a| + |b|) at most, turned by the rotation) and rounds its
    result again (2^-8 of it): together one bf16 ulp, 2^-7, of |a| + |b|."""
    T, hd, H, Hkv = g.Tq, g.hd, g.H, g.Hkv
    tab = ops.rope_table(T, hd, pos0=pos0)
    rope = (tab[..., 0].double().cpu(), tab[..., 1].double().cpu())
    c = A.case(g, "randn", rope=rope, rope_key=pos0)
    fused = [t.clone() for t in run_bwd(g, c, rope_tab=tab)]
    check_bwd(g, c, fused, f"{A.geo_id(g)} pos0={pos0} fused")
    plain = [t.clone() for t in run_bwd(g, c)]
    for i, heads in ((0, H), (1, Hkv)):
        x = plain[i].contiguous()
        pre = x.float().view(g.B * T, heads, 2, hd // 2).abs().sum(2, keepdim=True).expand(-1, -1, 2, -1).reshape(g.B * T, heads * hd)
        ops.rope_tab_(x, T, heads, hd, tab, inverse=True)
        diff = (x.float() - fused[i].float()).abs()
        over = diff > 2.0 ** -7 * pre
        assert not bool(over.any()), f"{'dq dk'.split()[i]}: {int(over.sum())} elements differ from the unfused sequence by more than one ulp"
    assert torch.equal(plain[2], fused[2])
    # the table exists in the bf16 MFMA kernels only
    with pytest.raises(ValueError):
        run_bwd(g, c, rope_tab=tab, impl=1)
    gf = g._replace(form="ref-f32", dt="f32", emul="ref")
    cf = A.case(gf, "randn")
    with pytest.raises(ValueError):
        run_bwd(gf, cf, rope_tab=tab)


# B * H > 1024 takes the 4-wave kernel, whose trip is 4 passes of 256 / (hd / 8) rows: 128 rows at hd 64, 64 at hd 128 -- one below, at, one above
DECODE_CASES = [g + (t,) for g in ((2, 4, 4, 128), (3, 8, 2, 64)) for t in (1, 64, 65, 257)] + \
               [(17, 64, 8, 64, t) for t in (1, 127, 128, 129)] + [(9, 128, 16, 128, t) for t in (1, 63, 64, 65)]


@pytest.mark.parametrize("fam", ["count", "offset"])
@pytest.mark.parametrize("B,H,Hkv,hd,Tk", DECODE_CASES)
def test_decode(dev, B, H, Hkv, hd, Tk, fam):
    """Single-query attention over a KV cache: no LSE comes back, so the count family checks the mean of the visible V alone (a row past Tk read, a
    row before it skipped or a wrong kv head is a wrong mean) and the offset family the general sum.  Cache rows past Tk are NaN."""
    g = A._g("decode", 1, hd, False, "ref", B=B, H=H, Hkv=Hkv, Tk=Tk)
    c = A.case(g, fam)
    Tmax = Tk + 3
    kc = torch.full((B, Tmax, Hkv * hd), float("nan"), dtype=torch.bfloat16)
    vc = kc.clone()
    kc[:, :Tk], vc[:, :Tk] = c.k.view(B, Tk, -1), c.v.view(B, Tk, -1)
    qd, kd, vd = c.q.cuda(), kc.cuda(), vc.cuda()
    o = ops.attention_decode(qd, kd, vd, H, Tk)
    bar = c.bar_o if fam == "count" else c.bar_o + Bar.attn_decode_weight_term(Tk, c.v)
    check(o, c.o64, bar, f"decode B{B} H{H} Hkv{Hkv} hd{hd} Tk{Tk} {fam}", "decode o")
    td = torch.tensor([Tk - 1], device=dev, dtype=torch.int32)
    assert torch.equal(ops.attention_decode(qd, kd, vd, H, 1, tk_dev=td), o)
