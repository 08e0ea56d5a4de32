"""Kernel-level parity of the memory-bound kernels (csrc/norm.hip, elementwise.hip, loss_optim.hip, connector_ops.hip) against the float64
restatements of tests/refs64.py, at model widths, every launch form and the edges.  Bars: tests/bars.py ("memory-bound kernels against
float64"); the fp32 measurement each bar starts from is made inside the case, on the host, from the same inputs.

Input families: randn; offset (mu + z: 30 and 1000 for fp32, 8 for bf16, which keeps sigma above bf16's spacing); heavy (channel 1 is 1e3 x the
rest: the massive activations of Whisper / Llama residual streams); tiny (1e-4 z: eps dominates the variance); const (every row one dyadic value:
variance exactly 0).

Pairs left out because they say nothing new, and nothing beyond these:
  * offset / const for the elementwise kernels (SwiGLU, act_residual, RoPE, cast ...): no reduction, so a shifted input is just another point of
    the [-100, 100] sweep, which they all get instead;
  * offset / heavy / tiny / const for RoPE: the rotation is linear in x, the position and frequency edges are what it is swept over;
  * families for cross entropy are its logit scales (1, 30, a +80 spike) and label patterns; for argmax its tie / inf / NaN rows;
  * the bit-exact movers take special values (NaN, +-inf, -0, bf16 ties) instead of families.
Sizes trimmed to keep the file near two minutes (the edge shapes all stay): 4099 rows only up to d = 2560; M = 512 instead of 2048 for
F >= 11008; B*T = 4096 only for V <= 1001; one AdamW step instead of 50 at n = 40 * 2^20; GroupNorm families and GELU at three shapes (one per width),
C = 4096 with T = 1500 at B = 1."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64 as R  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
DT = {"f32": F32, "bf16": BF16}
U = Bar.U32


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def family(name, rows, d, dtype, seed, dev="cuda"):
    """[rows, d] input of one family, rounded to `dtype` (the kernel and every reference see the same rounded values)."""
    z = torch.randn(rows, d, generator=gen(seed))
    if name == "randn":
        x = z
    elif name.startswith("offset"):
        x = float(name[6:]) + z
    elif name == "heavy":
        x = z.clone()
        x[:, 1 % d] *= 1e3
    elif name == "tiny":
        x = 1e-4 * z
    elif name == "const":
        r = torch.arange(rows)
        x = (0.5 * (r % 7 + 1).float() * (1 - 2 * (r % 2)).float())[:, None].expand(rows, d).contiguous()
    else:
        raise KeyError(name)
    return x.to(dtype).to(dev)


def families(dtype):
    return ["randn", "heavy", "tiny", "const"] + (["offset30", "offset1000"] if dtype == F32 else ["offset8"])


def check(out, ref64, bar, what):
    """max |out - ref64| <= bar (a number or an elementwise tensor), and no NaN / inf where the reference is finite."""
    o = out.detach().double().cpu()
    assert o.shape == ref64.shape, (what, o.shape, ref64.shape)
    fin = torch.isfinite(ref64)
    assert bool(torch.isfinite(o[fin]).all()), f"{what}: non-finite output where the reference is finite"
    err = (o - ref64).abs()
    bar_t = bar if torch.is_tensor(bar) else torch.full_like(err, float(bar))
    over = (err > bar_t) & fin
    worst = float((err / bar_t.clamp_min(1e-300))[fin].max()) if bool(fin.any()) else 0.0
    print(f"{what}: max err {float(err[fin].max()):.3e}, {worst:.3f} of the bar (max ref {float(ref64[fin].abs().max()):.3e})")
    assert not bool(over.any()), f"{what}: {int(over.sum())}/{err.numel()} beyond the bar, worst {worst:.2f}x (max err {float(err[fin].max()):.3e})"


def bar_of(ref64, cpu32, dtype, extra=0.0):
    b = Bar.fp32_bar(ref64, cpu32) + extra
    return Bar.bf16_bar(ref64, b) if dtype == BF16 else b


# ================================================================ norms
WIDTHS = [8, 64, 128, 768, 1024, 1280, 2048, 2052, 2560, 4096, 5120, 8192]          # every (VEC, NT) form and layernorm768_kernel
NORM_CASES = [(37, d, "randn") for d in WIDTHS]
NORM_CASES += [(rows, d, "randn") for d in (128, 768, 4096, 8192) for rows in (1, 3, 4)]
NORM_CASES += [(4099, d, "randn") for d in (128, 768, 2560)]
NORM_FAMILY_WIDTHS = (768, 1280, 2560, 5120)


def norm_cases():
    out = []
    for dn, dt in DT.items():
        out += [pytest.param(dt, r, d, f, id=f"{dn}-rows{r}-d{d}-{f}") for r, d, f in NORM_CASES]
        out += [pytest.param(dt, 5, d, f, id=f"{dn}-rows5-d{d}-{f}") for d in NORM_FAMILY_WIDTHS for f in families(dt) if f != "randn"]
    return out


def wb(d, dtype):
    w = (1 + 0.1 * torch.randn(d, generator=gen(14 + d))).to(dtype).cuda()
    b = (0.1 * torch.randn(d, generator=gen(15 + d))).to(dtype).cuda()
    return w, b


@pytest.mark.parametrize("dtype,rows,d,fam", norm_cases())
def test_layernorm(dev, dtype, rows, d, fam):
    x = family(fam, rows, d, dtype, 13)
    w, b = wb(d, dtype)
    ref = R.layernorm(x, w, b, 1e-5)
    cpu32 = F.layer_norm(x.float().cpu(), (d,), w.float().cpu(), b.float().cpu(), 1e-5)
    check(ops.layernorm(x, w, b, 1e-5), ref, bar_of(ref, cpu32, dtype), "layernorm")


@pytest.mark.parametrize("dtype,rows,d,fam", norm_cases())
def test_rmsnorm_fwd(dev, dtype, rows, d, fam):
    x = family(fam, rows, d, dtype, 13)
    w, _ = wb(d, dtype)
    ref, ref_rstd = R.rmsnorm_fwd(x, w, 1e-5)
    c32, c32_rstd = R.rmsnorm_fwd(x, w, 1e-5, dtype=F32)
    y, rstd = ops.rmsnorm_fwd(x, w, 1e-5)
    check(y, ref, bar_of(ref, c32, dtype), "rmsnorm_fwd y")
    check(rstd, ref_rstd, Bar.fp32_bar(ref_rstd, c32_rstd), "rmsnorm_fwd rstd")          # rstd is fp32 in both modes


@pytest.mark.parametrize("with_dres", [False, True], ids=["nodres", "dres"])
@pytest.mark.parametrize("dtype,rows,d,fam", norm_cases())
def test_rmsnorm_bwd(dev, dtype, rows, d, fam, with_dres):
    x = family(fam, rows, d, dtype, 13)
    w, _ = wb(d, dtype)
    dy = family("randn", rows, d, dtype, 16)
    dres = family("randn", rows, d, dtype, 17) if with_dres else None
    rstd = R.rmsnorm_fwd(x, w, 1e-5)[1].float().cuda()                                  # the forward's rstd, as the kernel takes it: fp32
    ref = R.rmsnorm_bwd(dy, x, w, rstd, dres)
    c32 = R.rmsnorm_bwd(dy, x, w, rstd, dres, dtype=F32)
    check(ops.rmsnorm_bwd(dy, x, w, rstd, dres), ref, bar_of(ref, c32, dtype), "rmsnorm_bwd")


@pytest.mark.parametrize("d", [6, 8196, 16384])
def test_norm_width_errors_before_any_launch(dev, d):
    """av_layernorm / av_rmsnorm_fwd / av_rmsnorm_bwd check d % 4 == 0 && d <= 8192 with AV_CHECK_ARG ahead of the launch: AV_ERR_ARG."""
    x, w = torch.zeros(2, d, device=dev), torch.ones(d, device=dev)
    for call in (lambda: ops.layernorm(x, w, w), lambda: ops.rmsnorm_fwd(x, w, 1e-5), lambda: ops.rmsnorm_bwd(x, x, w, torch.ones(2, device=dev))):
        with pytest.raises(ValueError, match="unsupported"):
            call()


# ================================================================ GroupNorm on tokens
GN_SHAPES = [(C_, G, T, B) for C_, G in ((64, 8), (1024, 32), (4096, 32)) for T in (1, 7, 375, 1500) for B in (1, 3)
             if not (C_ == 4096 and T == 1500 and B == 3)]


def gn_cases():
    out = []
    for dn, dt in DT.items():
        out += [pytest.param(dt, C_, G, T, B, "randn", 0, id=f"{dn}-C{C_}g{G}-T{T}-B{B}-randn-noact") for C_, G, T, B in GN_SHAPES]
        for C_, G, T, B in ((1024, 32, 375, 2), (64, 8, 7, 1), (4096, 32, 375, 1)):
            out += [pytest.param(dt, C_, G, T, B, f, act, id=f"{dn}-C{C_}g{G}-T{T}-B{B}-{f}-{'gelu' if act else 'noact'}")
                    for f in families(dt) + (["offset100s0.1"] if dt == F32 else []) for act in (0, 1) if not (f == "randn" and act == 0)]
    return out


@pytest.mark.parametrize("dtype,C_,G,T,B,fam,act", gn_cases())
def test_groupnorm_tokens(dev, dtype, C_, G, T, B, fam, act):
    if fam == "offset100s0.1":                                   # mu / sigma = 1e3 at mu = 100: one-pass E[x^2] - mean^2 in fp32 is off by 0.9 here
        x = (100 + 0.1 * torch.randn(B * T, C_, generator=gen(40))).to(dtype).cuda()
    elif fam == "const":                                         # one dyadic value per item: every (item, group) slab has variance exactly 0
        x = (0.5 * (torch.arange(B) % 7 + 1).float())[:, None].expand(B, T * C_).reshape(B * T, C_).to(dtype).cuda()
    else:
        x = family(fam, B * T, C_, dtype, 40)
    x = x.view(B, T, C_)
    w, b = wb(C_, dtype)
    ref = R.groupnorm_tokens(x, w, b, G, 1e-5, act)
    cpu32 = F.group_norm(x.float().cpu().transpose(1, 2), G, w.float().cpu(), b.float().cpu(), 1e-5).transpose(1, 2)
    if act:
        cpu32 = F.gelu(cpu32)
    check(ops.groupnorm_tokens(x, w, b, G, 1e-5, act), ref, bar_of(ref, cpu32, dtype), "groupnorm_tokens")


# ================================================================ RoPE
LLAMA32 = (32.0, 1.0, 4.0, 8192)                                 # Llama-3.2-1B's rope_scaling


def rope_bar(x64, T, heads, hd, ang, dtype, ref, ulps):
    """|a| + |b| of each rotated pair times the cos / sin error the angle bar allows, plus the three roundings of a c - b s."""
    rows = x64.shape[0]
    xv = x64.view(rows // T, T, heads, hd).abs()
    mag = xv[..., : hd // 2] + xv[..., hd // 2:]
    e = mag * (Bar.rope_angle_bar(ang.double(), ulps)[None, :, None, :] + 3 * U)
    bar = torch.cat([e, e], -1).reshape(rows, heads * hd)
    return bar + Bar.BF16_OUT_REL * ref.abs() if dtype == BF16 else bar


def rope_cases():
    """avllm_rope has no frequency-scaling argument: the llama3 rule exists in the table form only, so (direct, llama3) is not a case."""
    out = []
    for dn, dt in DT.items():
        for path in ("direct", "table", "table_posdev"):
            out += [pytest.param(dt, hd, th, None, path, id=f"{path}-{dn}-hd{hd}-theta{th:g}") for hd in (64, 128) for th in (1e4, 5e5, 1e6)]
            if path != "direct":
                out.append(pytest.param(dt, 64, 5e5, LLAMA32, path, id=f"{path}-{dn}-hd64-theta5e+05-llama3"))
    return out


@pytest.mark.parametrize("dtype,hd,theta,scaling,path", rope_cases())
def test_rope(dev, dtype, hd, theta, scaling, path):
    B, H = 2, 3
    ulps = Bar.rope_llama3_ulps(hd, theta, scaling)[None, :] if scaling else 4.0       # [1, hd/2] against the [T, hd/2] angles
    for pos0 in (0, 5, 2047, 8191, 131000):
        for T in (1, 19, 512):
            buf = torch.randn(B * T, 3 * H * hd, generator=gen(18 + T)).to(dtype).cuda()
            before = buf.clone()
            x = buf[:, H * hd: 2 * H * hd]                       # the k slice of a fused q|k|v buffer: row stride 3x the width
            pos = torch.arange(pos0, pos0 + T)
            ang = R.rope_angles(pos, hd, theta, scaling)

            def run(inverse):
                if path == "direct":
                    return ops.rope_(x, T, H, hd, pos0=pos0, theta=theta, inverse=inverse)
                from_dev = min(3, pos0) if path == "table_posdev" else None      # part of the position from device memory, as the token step passes it
                pd = torch.tensor([from_dev], device=dev, dtype=torch.int32) if from_dev is not None else None
                tab = ops.rope_table(T, hd, pos0 - (from_dev or 0), theta, pos_dev=pd, scaling=scaling)
                if not inverse:
                    tref = torch.stack([ang.double().cos(), ang.double().sin()], -1)
                    check(tab, tref, Bar.rope_angle_bar(ang.double(), ulps)[..., None].expand(T, hd // 2, 2), f"rope_table pos0={pos0} T={T}")
                return ops.rope_tab_(x, T, H, hd, tab, inverse=inverse)

            what = f"rope[{path}] pos0={pos0} T={T}"
            x64 = before[:, H * hd: 2 * H * hd].double().cpu()
            ref = R.rope(x64, T, H, hd, pos, theta, scaling)
            run(False)
            check(x, ref, rope_bar(x64, T, H, hd, ang, dtype, ref, ulps), what)
            ref64 = R.rope(x64, T, H, hd, pos, theta, scaling, hf=False)
            print(f"{what}: (information) distance of the HF-angle reference from the float64-angle one {float((ref - ref64).abs().max()):.3e}")
            assert torch.equal(buf[:, : H * hd], before[:, : H * hd]) and torch.equal(buf[:, 2 * H * hd:], before[:, 2 * H * hd:]), f"{what}: q / v slices touched"
            x.copy_(before[:, H * hd: 2 * H * hd])
            iref = R.rope(x64, T, H, hd, pos, theta, scaling, inverse=True)
            run(True)
            check(x, iref, rope_bar(x64, T, H, hd, ang, dtype, iref, ulps), what + " inverse")


# ================================================================ SwiGLU / act_residual
SPECIALS = [0.0, -0.0, -88.0, -104.0, 88.0, 104.0, -100.0, 100.0, 1e-40, -1e-40, 1.4e-45, -87.5, -89.0, -103.0]
MF = [(1, 4), (33, 4), (2048, 4), (1, 192), (33, 192), (2048, 192), (1, 11008), (33, 11008), (512, 11008), (1, 14336), (33, 14336), (512, 14336)]


def sweep(rows, d, dtype, seed):
    """Arguments over [-100, 100] with the fp32 exp overflow points, signed zeros and denormals among them."""
    n = rows * d
    x = torch.rand(n, generator=gen(seed)) * 200 - 100
    sp = torch.tensor(SPECIALS)
    idx = torch.arange(0, n, max(1, n // 64))[: len(SPECIALS) * 4]
    x[idx] = sp[torch.arange(idx.numel()) % len(SPECIALS)]
    return x.view(rows, d).to(dtype).cuda()


def ew_cases():
    out = []
    for dn, dt in DT.items():
        out += [pytest.param(dt, M, F_, "sweep", id=f"{dn}-M{M}-F{F_}-sweep") for M, F_ in MF]
        out += [pytest.param(dt, M, F_, f, id=f"{dn}-M{M}-F{F_}-{f}") for M, F_ in ((33, 192), (512, 11008)) for f in ("randn", "heavy", "tiny")]
    return out


def ew_input(fam, M, F_, dtype, seed):
    return sweep(M, F_, dtype, seed) if fam == "sweep" else family(fam, M, F_, dtype, seed)


@pytest.mark.parametrize("dtype,M,F_,fam", ew_cases())
def test_swiglu(dev, dtype, M, F_, fam):
    gu = torch.cat([ew_input(fam, M, F_, dtype, 19), family("randn", M, F_, dtype, 20)], 1)
    g, u = gu[:, :F_].double().cpu(), gu[:, F_:].double().cpu()
    ref = R.swiglu_fwd(gu)
    bar = Bar.silu_bar(g) * u.abs() + U * ref.abs() + Bar.FP32_DENORM
    check(ops.swiglu_fwd(gu), ref, bar + Bar.BF16_OUT_REL * ref.abs() if dtype == BF16 else bar, "swiglu_fwd")
    dh = family("randn", M, F_, dtype, 21)
    refb = R.swiglu_bwd(dh, gu)
    barb = Bar.swiglu_bwd_bar(dh.double().cpu(), g, u)
    check(ops.swiglu_bwd(dh, gu), refb, barb + Bar.BF16_OUT_REL * refb.abs() if dtype == BF16 else barb, "swiglu_bwd")


@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", [L.ACT_GELU, L.ACT_QUICK_GELU, L.ACT_SILU], ids=["gelu", "quickgelu", "silu"])
@pytest.mark.parametrize("dtype,M,F_,fam", ew_cases())
def test_act_residual(dev, dtype, M, F_, fam, act, res):
    x = ew_input(fam, M, F_, dtype, 22)
    r = family("randn", M, F_, dtype, 23) if res else None
    ref = R.activation(x, act, r)
    if act == L.ACT_GELU:                                        # erff, no fast exponential: the measured-fp32 bar
        c32 = F.gelu(x.float().cpu()) + (r.float().cpu() if res else 0)
        bar = Bar.fp32_bar(ref, c32)
    else:
        bar = Bar.silu_bar(x.double().cpu(), 1.702 if act == L.ACT_QUICK_GELU else 1.0) + U * ref.abs()
    check(ops.act_residual(x, act, r), ref, bar + Bar.BF16_OUT_REL * ref.abs() if dtype == BF16 else bar, "act_residual")


# ================================================================ cross entropy
CE_SHAPES = [(V, V, B, T) for V in (8, 1000) for B, T in ((1, 1), (2, 40), (2, 2048))] + \
            [(V, V, B, T) for V in (32000, 128256) for B, T in ((1, 1), (2, 40))] + \
            [(1001, 1008, B, T) for B, T in ((1, 1), (2, 40), (2, 2048))] + [(32003, 32008, B, T) for B, T in ((1, 1), (2, 40))]
PATTERNS = ["all", "none", "last_only", "edge_ids", "beyond_vocab"]


def ce_cases():
    out = []
    for dn, dt in DT.items():
        for V, ld, B, T in CE_SHAPES:
            for sc in (1, 30):
                pats = PATTERNS if (B * T == 80 and V in (8, 1000, 1001, 32003) and sc == 30) else ["all"]
                out += [pytest.param(dt, V, ld, B, T, sc, p, id=f"{dn}-V{V}ld{ld}-B{B}T{T}-scale{sc}-{p}") for p in pats]
    return out


def ce_labels(pat, B, T, V):
    lab = torch.randint(0, V, (B, T), generator=gen(26))
    if pat == "none":
        lab[:] = -100
    elif pat == "last_only":                                     # the shift scores row T-2 against it; position 0's label is never used
        lab[:] = -100
        lab[:, T - 1] = 1 % V
        lab[0, 0] = 0
    elif pat == "edge_ids":
        lab[:, 0::2] = V - 1
        lab[:, 1::2] = 0
    elif pat == "beyond_vocab":
        lab[:, 1::3] = V
        lab[:, 2::3] = V + 12345
    return lab.cuda()


@pytest.mark.parametrize("dtype,V,ld,B,T,scale,pat", ce_cases())
def test_cross_entropy(dev, dtype, V, ld, B, T, scale, pat):
    raw = (torch.randn(B, T, ld, generator=gen(25)) * scale)
    if B * T >= 80:
        raw[1, 5, V - 2] += 80.0                                 # a spike in the row's last vector: the running maximum jumps at the very end
    buf = raw.to(dtype).cuda()
    buf[:, :, V:] = 7.0                                          # padding columns (ld > V): never read, never written
    logits = buf[:, :, :V]
    labels = ce_labels(pat, B, T, V)
    gs = 0.37
    ref_lse, ref_sum, ref_cnt, ref_g = R.cross_entropy(logits, labels, grad_scale=gs)
    row_lse, acc = ops.ce_fwd(logits, labels)
    x64 = logits.double().cpu()
    lse_bar = Bar.fp32_bar(ref_lse, torch.logsumexp(logits.float().cpu(), -1).reshape(-1)) + Bar.ce_lse_expf_term(V)
    check(row_lse, ref_lse, lse_bar, "ce_fwd row_lse")
    assert float(acc[1]) == ref_cnt, (float(acc[1]), ref_cnt)
    if ref_cnt == 0:
        assert float(acc[0]) == 0.0
    else:                                                        # atomics in any order: gamma_n sum|terms| for the accumulation, n lse bars for the terms
        terms = float((ref_lse.abs().max() + x64.abs().max()))
        sum_bar = ref_cnt * (lse_bar + U * terms) + ref_cnt * U * float(ref_sum)         # every term lse - x[target] is >= 0: sum |terms| = the sum
        print(f"ce_fwd loss_sum: err {abs(float(acc[0]) - float(ref_sum)):.3e}, bar {sum_bar:.3e}, sum {float(ref_sum):.6e}")
        assert abs(float(acc[0]) - float(ref_sum)) <= sum_bar
    # gradient: g (exp(x - lse) - onehot); the kernel's own fp32 lse enters through exp: relative error lse_bar on p.  (p - onehot) g carries four
    # roundings: grad_scale to fp32, g = grad_scale / count, the subtraction, the product
    dl = ops.ce_bwd(logits, labels, row_lse, acc, grad_scale=gs)
    assert dl.stride() == logits.stride()
    if ref_cnt == 0:
        assert float(dl.float().abs().max()) == 0.0 and not bool(torch.isnan(dl.float()).any())
    else:
        a = x64 - ref_lse.view(B, T, 1)
        p = a.exp()
        oh = ref_g * (ref_cnt / gs) - p                          # -(onehot) on scored rows; on unscored rows ref_g is 0 and the row's bar is 0 + the floor
        scored = (ref_g.abs().sum(-1, keepdim=True) > 0).double()
        bar = (gs / ref_cnt) * scored * (p * (3 * a.abs() * U + 2 * U + lse_bar) + 4 * U * (p + oh).abs()) + Bar.FP32_DENORM
        check(dl, ref_g, bar + Bar.BF16_OUT_REL * ref_g.abs() if dtype == BF16 else bar, "ce_bwd")
    inplace = buf.clone()
    lv = inplace[:, :, :V]
    out = ops.ce_bwd(lv, labels, row_lse, acc, grad_scale=gs, out=lv)
    assert out.data_ptr() == lv.data_ptr()
    assert torch.equal(lv.view(torch.int16 if dtype == BF16 else torch.int32), dl.view(torch.int16 if dtype == BF16 else torch.int32)), "in place != out of place"
    assert bool((inplace[:, :, V:] == 7.0).all()) and bool((buf[:, :, V:] == 7.0).all()), "padding columns written"


def test_ce_bwd_rejects_what_it_cannot_address(dev):
    logits = torch.zeros(2, 4, 16, device=dev)
    labels = torch.zeros(2, 4, dtype=torch.int64, device=dev)
    row_lse, acc = ops.ce_fwd(logits, labels)
    with pytest.raises(ValueError, match="out must have"):
        ops.ce_bwd(logits[:, :, :9], labels, row_lse, acc, out=torch.empty(2, 4, 9, device=dev))       # dense out for a padded view
    with pytest.raises(ValueError, match="rows of one stride"):
        ops.ce_bwd(torch.zeros(2, 4, 9, device=dev), labels, row_lse, acc)                            # row stride 9: not a multiple of 8


# ================================================================ argmax
@pytest.mark.parametrize("V", [1, 255, 256, 257, 32000, 128256])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_argmax_rows(dev, dtype, V):
    """Rule (refs64.argmax_rows): the lowest index of the maximum with NaN read as -inf: torch.argmax on every row without NaN, 0 for a row of
    all -inf / NaN, always in [0, V).  Kernel level only: generate() is never driven with non-finite logits."""
    inf, nan = float("inf"), float("nan")
    ties = [[V - 1, 0], [255, 256], [256, 257], [257, 511, 512], [V - 1, V - 2], [300, 44], [V // 2, V // 2 + 256], [1023, 1024, 767]]
    rows = []
    for i, t in enumerate(ties):                                 # exact ties of the maximum across thread (c % 256) and stride (c / 256) boundaries
        r = torch.randn(V, generator=gen(50 + i))
        r[torch.tensor([c for c in t if 0 <= c < V] or [0], dtype=torch.int64)] = 9.0
        rows.append(r)
    r = torch.randn(V, generator=gen(60)); r[torch.tensor([c for c in (V - 1, 256, 3) if c < V])] = inf; rows.append(r)           # +inf ties
    rows.append(torch.full((V,), -inf))                                                                               # all -inf -> 0
    r = torch.full((V,), -inf); r[V - 1] = -3.0e38; rows.append(r)
    r = torch.randn(V, generator=gen(61)); r[torch.tensor([c for c in (V - 1, 700, 2) if c < V])] = nan; r[0] = inf; rows.append(r)     # NaN after a +inf
    rows.append(torch.full((V,), nan))
    r = torch.full((V,), -inf); r[V // 2] = nan; rows.append(r)
    rows.append(torch.randn(V, generator=gen(62)))
    x = torch.stack(rows).to(dtype)
    buf = torch.full((x.shape[0], (V + 8 + 7) // 8 * 8), inf, dtype=dtype, device=dev)          # padded row stride; +inf in the padding must not be seen
    buf[:, :V] = x.cuda()
    got = ops.argmax_rows(buf[:, :V]).cpu()
    exp = R.argmax_rows(x)
    assert bool(((got >= 0) & (got < V)).all()), got.tolist()
    assert torch.equal(got, exp), (got.tolist(), exp.tolist())
    nonan = ~torch.isnan(x.float()).any(-1)
    assert torch.equal(got[nonan], torch.argmax(x.float(), -1)[nonan])


# ================================================================ gradient norm / AdamW / schedule
NS = [1, 3, 4, 5, 1023, 2 ** 20 + 3, 40 * 2 ** 20]


@pytest.mark.parametrize("n", NS)
def test_grad_sumsq(dev, n):
    g = torch.randn(n, generator=gen(70)).cuda() * 0.3
    ref = (g.double() ** 2).sum().cpu().reshape(1)
    bar = Bar.fp32_bar(ref, (g.cpu() ** 2).sum().reshape(1))
    blocks = max(1, min(1024, (n // 4 + 255) // 256))            # av_grad_sumsq's grid: one float atomic per block, in arrival order
    abar = bar + Bar.atomic_sum_term(blocks, float(ref))
    out = torch.zeros(1, device=dev)
    ops.grad_sumsq(g, out)
    check(out, ref, abar, "grad_sumsq")
    ops.grad_sumsq(g, out)                                       # accumulates
    check(out, 2 * ref, 2 * bar + Bar.atomic_sum_term(2 * blocks, 2 * float(ref)), "grad_sumsq twice")
    dets = []
    for nparts in (1024, 1024, 7, 1):
        parts, o = torch.full((nparts,), float("nan"), device=dev), torch.full((1,), 123.0, device=dev)      # overwrites, reads no stale partial
        ops.grad_sumsq(g, o, partials=parts)
        check(o, ref, bar, f"grad_sumsq_det nparts={nparts}")
        dets.append(o.clone())
    assert torch.equal(dets[0], dets[1]), "the fixed-order sum must repeat bit for bit"


def read_state(state):
    return L.StepState.from_buffer_copy(bytes(state.cpu().numpy().tobytes()))


def new_state(dev, step=0, skipped=0.0):
    st = L.StepState()
    st.step, st.skipped = step, skipped
    return torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).clone().to(dev)


def adamw_cases():
    """n = 40 * 2^20 runs one step of one configuration (clip + prescale + decay); every configuration runs 50 steps at every smaller n."""
    cfgs = {"clip-wd": (0.5, 1.0, 0.01), "noclip-nowd": (0.0, 1.0, 0.0), "clip-prescale-wd": (0.5, 0.125, 0.01), "noclip-prescale-wd": (0.0, 4.0, 0.01)}
    return [pytest.param(n, *c, id=f"n{n}-{k}") for n in NS for k, c in cfgs.items() if n <= 2 ** 20 + 3 or k == "clip-prescale-wd"]


@pytest.mark.parametrize("n,max_norm,prescale,wd", adamw_cases())
def test_adamw(dev, n, max_norm, prescale, wd):
    steps = 50 if n <= 2 ** 20 + 3 else 1
    lr0 = 3e-3
    p0 = torch.randn(n, generator=gen(71))
    p, m, v = p0.cuda(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p32, m32, v32 = p0.clone(), torch.zeros(n), torch.zeros(n)
    parts, ss = torch.zeros(1024, device=dev), torch.zeros(1, device=dev)
    for s in range(1, steps + 1):
        g = (torch.randn(n, generator=gen(1000 + s)) * (0.3 / prescale)).cuda()
        lr = R.schedule(s, lr0, 60)[0]
        ops.grad_sumsq(g, ss, partials=parts)
        ops.adamw_step(p, g, m, v, lr, s, sumsq=ss, max_norm=max_norm, prescale=prescale, wd=wd)
        gc = g.cpu()
        coef = R.clip_coef(float((gc.double() ** 2).sum()), max_norm, prescale)
        R.adamw_step(p64, gc.double(), m64, v64, lr, s, coef=coef, wd=wd)
        R.adamw_step(p32, gc, m32, v32, lr, s, coef=coef, wd=wd)                       # the same rule in fp32 on the host: the bar's measurement
    check(p, p64, Bar.fp32_bar(p64, p32), f"adamw p after {steps} steps")
    check(m, m64, Bar.fp32_bar(m64, m32), "adamw m")
    check(v, v64, Bar.fp32_bar(v64, v32), "adamw v")


@pytest.mark.parametrize("use_state", [False, True], ids=["scalars", "state"])
@pytest.mark.parametrize("bad", ["sumsq_inf", "sumsq_nan", "guard_nan", "guard_inf"])
def test_adamw_skips_non_finite_step(dev, bad, use_state):
    n = 1023
    p, g = torch.randn(n, generator=gen(72)).cuda(), torch.randn(n, generator=gen(73)).cuda()
    m, v = torch.rand(n, generator=gen(74)).cuda(), torch.rand(n, generator=gen(75)).cuda()
    keep = [t.clone() for t in (p, m, v)]
    ss = torch.tensor([float("inf") if bad == "sumsq_inf" else float("nan") if bad == "sumsq_nan" else 1.0], device=dev)
    guard = torch.tensor([float("nan") if bad == "guard_nan" else float("-inf") if bad == "guard_inf" else 2.0], device=dev)
    skipped = torch.zeros(1, device=dev)
    state = None
    if use_state:
        state = new_state(dev)
        for _ in range(3):
            ops.step_advance(state, 1e-3, 100)
    ops.adamw_step(p, g, m, v, 1e-3, 3, sumsq=ss, max_norm=0.5, guard=guard, skipped=skipped, state=state)
    for a, b in zip((p, m, v), keep):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "a skipped step must leave p, m, v bit-identical"
    assert float(skipped) == 1.0
    if use_state:
        st = read_state(state)
        assert st.step == 2 and st.skipped == 1.0
        ops.step_advance(state, 1e-3, 100)                       # the retried step: same number, fresh dropout masks
        st = read_state(state)
        assert st.step == 3 and st.dropout_seed == R.dropout_seed(3, 1)
        ss.fill_(1.0); guard.fill_(2.0)
        ops.adamw_step(p, g, m, v, 123.0, 77, sumsq=ss, max_norm=0.0, guard=guard, skipped=skipped, state=state)      # lr / step arguments ignored
        p64, m64, v64 = (t.double().cpu() for t in keep)
        R.adamw_step(p64, g.double().cpu(), m64, v64, float(st.lr), 3, bc1=float(st.bc1), bc2_sqrt=float(st.bc2_sqrt))
        p32, m32, v32 = (t.cpu().clone() for t in keep)
        R.adamw_step(p32, g.cpu(), m32, v32, float(st.lr), 3, bc1=float(st.bc1), bc2_sqrt=float(st.bc2_sqrt))
        check(p, p64, Bar.fp32_bar(p64, p32), "adamw from step_state")
        assert float(skipped) == 1.0


@pytest.mark.parametrize("warm,total", [(0, 20000), (500, 20000), (0, 1000), (100, 1000)])
def test_step_advance(dev, warm, total):
    """lr, bc1, bc2_sqrt at sampled steps 1 .. 20 000 (beyond total_steps for the short schedules) against the float64 schedule.  Bar: the fp32
    evaluation of the same formula on the host (refs64.schedule(f32=True)) against float64, measured here over the same steps, x 4, floored at
    2 ulp of base_lr / of 1."""
    base = 5e-5
    steps = sorted(set(list(range(1, 40)) + [warm, warm + 1, warm + 2, total // 2, total - 1, total, total + 1, total + 2, 2 * total, 19999, 20000]
                       + list(range(97, 20001, 331))) - {0})
    e32 = [0.0, 0.0, 0.0]
    for s in steps:
        a, b = R.schedule(s, base, total, warm, f32=True), R.schedule(s, base, total, warm)
        e32 = [max(e, abs(x - y)) for e, x, y in zip(e32, a, b)]
    bars = [max(4 * e32[0], 4 * U * base), max(4 * e32[1], 4 * U), max(4 * e32[2], 4 * U)]
    worst = [0.0, 0.0, 0.0]
    state = new_state(dev)
    for s in steps:
        state.view(torch.int32)[0] = s - 1
        ops.step_advance(state, base, total, warm)
        st = read_state(state)
        assert st.step == s and st.dropout_seed == R.dropout_seed(s, 0)
        got, ref = (st.lr, st.bc1, st.bc2_sqrt), R.schedule(s, base, total, warm)
        worst = [max(w, abs(x - y)) for w, x, y in zip(worst, got, ref)]
    print(f"step_advance warm={warm} total={total}: measured |lr, bc1, bc2_sqrt - float64| = {worst}, fp32-on-host {e32}, bars {bars}")
    assert all(w <= b for w, b in zip(worst, bars)), (worst, bars)
    seq = new_state(dev)                                         # and consecutively, as the trainer calls it
    for s in range(1, 51):
        ops.step_advance(seq, base, total, warm, rank=2)
        st = read_state(seq)
        assert st.step == s and st.dropout_seed == R.dropout_seed(s, 0, rank=2)
        assert abs(st.lr - R.schedule(s, base, total, warm)[0]) <= bars[0]


# ================================================================ movers that must be bit-exact
def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b, what):
    """Bit-identical, except that a NaN may be any NaN."""
    a, b = a.cpu(), b.cpu()
    na, nb = torch.isnan(a.float()), torch.isnan(b.float())
    assert torch.equal(na, nb), f"{what}: NaN positions differ"
    assert torch.equal(bits(a)[~na], bits(b)[~nb]), f"{what}: {int((bits(a)[~na] != bits(b)[~nb]).sum())} values differ in bits"


def special_values(n, dtype, seed):
    x = torch.randn(n, generator=gen(seed))
    sp = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20,
                       1 + 2.0 ** -8 - 2.0 ** -20, 3.3895e38, 1e-40, 65280.0 + 128.0])          # bf16 ties (to even, both ways), just above / below a tie
    k = min(n, sp.numel())
    x[torch.randperm(n, generator=gen(seed + 1))[:k]] = sp[:k]
    return x.to(dtype)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 1021, 1022, 1023, 1024, 2 ** 20 + 1])
@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)], ids=["f32-bf16", "bf16-f32", "f32-f32", "bf16-bf16"])
def test_cast(dev, src, dst, n):
    x = special_values(n, src, 80).cuda()
    out = torch.empty(n, device=dev, dtype=dst)
    L.check(L.load().avllm_cast(L.ptr(x), L.dt_of(x), L.ptr(out), L.dt_of(out), n, L.stream_ptr()))
    same_bits(out, x.cpu().to(dst), f"cast n={n}")                # torch's host conversion: round to nearest even


@pytest.mark.parametrize("d", [32, 4096])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_embedding(dev, dtype, d):
    rows = 50
    table = special_values(rows * d, dtype, 81).view(rows, d).cuda()
    ids = torch.tensor([[0, rows - 1, 0, 7], [rows - 1, rows - 1, 1, 0]], device=dev)
    same_bits(ops.embedding(table, ids), table[ids], "embedding")


@pytest.mark.parametrize("pos", ["start", "end"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_kv_append(dev, dtype, pos):
    B, T, Tmax, d = 3, 5, 16, 64
    pos0 = 0 if pos == "start" else Tmax - T
    qkv = special_values(B * T * 3 * d, dtype, 82).view(B * T, 3 * d).cuda()
    kc, vc = special_values(B * Tmax * d, dtype, 83).view(B, Tmax, d).cuda(), special_values(B * Tmax * d, dtype, 84).view(B, Tmax, d).cuda()
    ek, ev = R.kv_append(kc, vc, qkv[:, d:2 * d], qkv[:, 2 * d:], B, T, pos0)
    ops.kv_append(qkv[:, d:2 * d], qkv[:, 2 * d:], kc, vc, T, pos0)
    same_bits(kc, ek, "kv_append k (appended rows and every untouched row)")
    same_bits(vc, ev, "kv_append v")
    with pytest.raises(ValueError, match="kv_append"):           # AV_CHECK_ARG ahead of the launch
        ops.kv_append(qkv[:, d:2 * d], qkv[:, 2 * d:], kc, vc, T, Tmax - T + 1)


@pytest.mark.parametrize("T", [1, 7, 8, 375])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_im2col_k3(dev, dtype, stride, T):
    B, Cc = 2, 24
    x = special_values(B * T * Cc, dtype, 85).view(B, T, Cc).cuda()
    To = (T - 1) // stride + 1
    cols = torch.full((B * To, 3 * Cc), 5.0, device=dev, dtype=dtype)
    L.check(L.load().avllm_im2col_k3(L.ptr(x), L.ptr(cols), B, T, Cc, stride, L.dt_of(x), L.stream_ptr()))
    same_bits(cols, R.im2col_k3(x, stride), "im2col_k3")
    fin = torch.nan_to_num(x.float().cpu(), nan=0.0, posinf=1.0, neginf=-1.0)             # F.unfold's own order, on finite values (unfold pads by arithmetic)
    u = F.unfold(fin.transpose(1, 2)[:, :, None, :], (1, 3), padding=(0, 1), stride=(1, stride)).view(B, Cc, 3, To).permute(0, 3, 2, 1).reshape(B * To, 3 * Cc)
    assert torch.equal(torch.nan_to_num(cols.float().cpu(), nan=0.0, posinf=1.0, neginf=-1.0), u)


class PackItem(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("A_pad", C.c_void_p), ("AT_pad", C.c_void_p), ("B_pad", C.c_void_p), ("BT_pad", C.c_void_p),
                ("ld_at", C.c_int64), ("dout", C.c_int64)]


@pytest.mark.parametrize("ld_at", [64, 192])
@pytest.mark.parametrize("r", [8, 16, 64])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_lora_pack(dev, dtype, r, ld_at):
    din, dout, P = 136, 200, L.LORA_PAD
    A = special_values(r * din, F32, 86).view(r, din).cuda()
    Bm = special_values(dout * r, F32, 87).view(dout, r).cuda()

    def images(fill):
        return [torch.full(s, fill, device=dev, dtype=dtype) for s in ((P, din), (din, ld_at), (dout, P), (P, dout))]

    Ap, ATp, Bp, BTp = images(5.0)                               # the single form writes the padding itself
    L.check(L.load().avllm_lora_pack(L.ptr(A), L.ptr(Bm), r, din, dout, L.ptr(Ap), L.ptr(ATp), ld_at, L.ptr(Bp), L.ptr(BTp), L.dt_of(Ap), L.stream_ptr()))
    eA = torch.zeros(P, din, dtype=dtype); eA[:r] = A.cpu().to(dtype)
    eB = torch.zeros(dout, P, dtype=dtype); eB[:, :r] = Bm.cpu().to(dtype)
    same_bits(Ap, eA, "A_pad"); same_bits(Bp, eB, "B_pad")
    same_bits(ATp[:, :P], eA.t().contiguous(), "AT_pad = A_pad^T"); same_bits(BTp, eB.t().contiguous(), "BT_pad = B_pad^T")
    assert bool((ATp[:, P:] == 5.0).all()), "columns of a shared [din, 192] image that belong to the other adapters were written"
    for name, img in (("A_pad", Ap[r:]), ("AT_pad", ATp[:, r:P]), ("B_pad", Bp[:, r:]), ("BT_pad", BTp[r:])):
        assert img.numel() == 0 or bool((bits(img) == 0).all()), f"{name}: padding is not +0"
    bA, bAT, bB, bBT = images(0.0)                               # the batch form rewrites the r real rows of zero-initialised images
    it = PackItem(L.ptr(A), L.ptr(Bm), L.ptr(bA), L.ptr(bAT), L.ptr(bB), L.ptr(bBT), ld_at, dout)
    items = torch.frombuffer(bytearray(bytes(it)), dtype=torch.uint8).clone().to(dev)
    L.check(L.load().avllm_lora_pack_batch(L.ptr(items), 1, r, din, L.dt_of(bA), L.stream_ptr()))
    torch.cuda.synchronize()
    same_bits(bA, Ap, "batch A_pad"); same_bits(bAT[:, :P], ATp[:, :P], "batch AT_pad"); same_bits(bB, Bp, "batch B_pad"); same_bits(bBT, BTp, "batch BT_pad")
    assert bool((bAT[:, P:] == 0).all())
