"""avllm_dec_proj, the fused projection of the token step, pinned elementwise to float64 in its three modes, three weight forms, three
activation-load forms, with and without the norm fold, the residual and adapters, at every length of the K ring's tails.

The comparison is (err <= bar).all() over every element against refs64_decode.dec_proj64; the bar is bars.dec_proj_bar, derived in bars.py from the
kernel's documented arithmetic and from nothing the kernel returns.  `exact` and `locate` carry the bar 0 wherever no rstd is involved (f32
output compared with torch.equal) and the rstd terms alone where the norm is folded.  Every case prints its worst err / bar.  The cases are
refs64_decode's lists; tests/test_decode_refs_cpu.py runs the host emulation and its mutants over the same lists, so what these tests can and
cannot see is known without a GPU."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars  # noqa: E402
import refs64_decode as D  # noqa: E402
from avllm import ops  # noqa: E402

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TMAX, POS = 5, 3


def dev_args(c):
    """The device-side keyword arguments of ops.dec_proj for a host case (weights apart)."""
    kw = dict(mode=c["mode"])
    if c.get("g") is not None:
        kw.update(norm_w=c["g"].to(BF).cuda(), eps=c["eps"])
    if c.get("bias") is not None:
        kw["bias"] = c["bias"].to(BF).cuda()
    if c.get("lt") is not None:
        kw.update(lora_t=c["lt"].cuda(), lora_b=[b.to(BF).cuda() for b in c["lbs"]], lora_r=c["r"], lora_scale=c["scale"])
    return kw


def weights_of(cache, W, form):
    """One upload (and fp8 quantisation) per distinct host matrix of a test."""
    key = (id(W), form)
    if key not in cache:
        wa = D.wargs(W, form)
        cache[key] = (W, wa.pop("W"), wa)
    return cache[key][1], cache[key][2]


def run_plain(c, Wd, wa):
    kw = dev_args(c)
    A = c["A"].to(BF).cuda()
    if c.get("R") is None:
        return ops.dec_proj(A, Wd, out_f32=c["out_f32"], **kw, **wa).double().cpu()
    R = c["R"].to(BF).cuda()
    if c["out_f32"]:
        return ops.dec_proj(A, Wd, R=R, out_f32=True, **kw, **wa).double().cpu()
    return ops.dec_proj(A, Wd, R=R, out=R, **kw, **wa).double().cpu()          # in place: out aliases R


def run_qkv(c, Wd, wa, pos=POS, pos_dev=None, tmax=TMAX):
    """-> (q | k row | v row at pos + *pos_dev as one [M, N] tensor, the cache rows elsewhere unchanged bit for bit)."""
    M, dq, dkv = c["A"].shape[0], c["dq"], c["dkv"]
    kc = torch.randn(M, tmax, dkv, generator=D.gen("kc", M, dkv)).to(BF).cuda()
    vc = torch.randn(M, tmax, dkv, generator=D.gen("vc", M, dkv)).to(BF).cuda()
    kc0, vc0 = kc.clone(), vc.clone()
    pd = None if pos_dev is None else torch.tensor([pos_dev], dtype=torch.int32, device="cuda")
    q = ops.dec_proj(c["A"].to(BF).cuda(), Wd, rope=c["rope"].cuda(), kc=kc, vc=vc, pos=pos, pos_dev=pd, dq=dq, dkv=dkv, hd=c["hd"], **dev_args(c), **wa)
    row = pos + (pos_dev or 0)
    keep = [t for t in range(tmax) if t != row]
    untouched = torch.equal(kc[:, keep], kc0[:, keep]) and torch.equal(vc[:, keep], vc0[:, keep])
    return torch.cat([q, kc[:, row], vc[:, row]], 1).double().cpu(), untouched


def held(got, ref, exact, tag, worst):
    """Elementwise comparison; asserts, and keeps the worst err / bar of the parametrised case: worst[0] over the f32 outputs, worst[1] over the bf16
    outputs (where the half spacing of the one rounding, up to 2^-8 |out| just above a power of two, is most of the bar)."""
    err = (got - ref.out).abs()
    if exact and ref.rstd is None and ref.out_f32:
        assert torch.equal(got, ref.out), f"{tag}: exact family differs by {float(err.max()):.3e} at {int(err.argmax())}"
        return
    bar = bars.dec_proj_bar(ref, exact=exact)
    ratio = err / bar
    i = 0 if ref.out_f32 else 1
    worst[i] = max(worst[i], float(ratio.max()))
    bad = int(ratio.argmax())
    assert bool((err <= bar).all()), f"{tag}: err {float(err.flatten()[bad]):.3e} over bar {float(bar.flatten()[bad]):.3e} at element {bad} (M x N = {tuple(got.shape)})"


# ------------------------------------------------------------------------------------------------ mode 0: the K deal, the ring, the AL boundaries
@pytest.mark.parametrize("form", D.FORMS)
@pytest.mark.parametrize("K", D.K_DEAL)
def test_plain_every_tail_and_row_count(dev, K, form):
    """N = 48 (three workgroups); M over the activation-load boundaries; norm off, on, on with a residual (in place where the output is bf16);
    exact / randn / offset / heavy.  offset's residual is -z + noise: a second rounding would leave 2^-9 |z| in a result of size 1."""
    cache, worst = {}, [0.0, 0.0]
    for cid, c, exact in D.plain_cases(K):
        Wd, wa = weights_of(cache, c["W"], form)
        held(run_plain(c, Wd, wa), D.dec_proj64(**c), exact, cid, worst)
    print(f"plain K={K} {form}: worst err/bar f32 out {worst[0]:.3e}, bf16 out {worst[1]:.3e}")


@pytest.mark.parametrize("form", D.FORMS)
@pytest.mark.parametrize("K", D.K_DEAL)
def test_locate_names_the_column_and_k(dev, K, form):
    """One-hot rows: row m of launch l is hot at k = 128 g + M l + m, ceil(128 / M) launches cover the whole group g (the first, a middle and the
    last group, in different waves); the weights differ wherever a slip could look (refs64_decode.locate_weights), so out[m, n] = W[n, k] g[k]
    names the element multiplied.  f32 output, bar 0 without the norm; with it (power-of-two norm weights that differ between a lane's steps)
    the rstd terms alone.  The walk itself is refs64_decode.locate_check, which the CPU file runs over the host emulation."""
    W = D.locate_weights(D.N_PLAIN, K)
    wa = D.wargs(W, form)
    Wd = wa.pop("W")
    gd = D.step_norm(K).to(BF).cuda()

    def run(A, norm):
        Ad = A.to(BF).cuda()
        kw = dict(norm_w=gd, eps=D.EPS) if norm else {}
        return torch.stack([ops.dec_proj(Ad[l], Wd, out_f32=True, **kw, **wa) for l in range(A.shape[0])]).double().cpu()
    worst = D.locate_check(run, K)
    print(f"locate K={K} {form}: worst err/bar of the normed launches {worst:.3e}")


@pytest.mark.parametrize("form", D.FORMS)
def test_forced_activation_load_forms_are_bit_identical(dev, form):
    """The DEC_AL knob forces the wider activation-load forms (2 and 4 at M = 1 and 3, 4 at M = 5; for fp4 the form 4 also has the shallower
    ring): the same elements meet in the same order, so the bytes are those of the default form, in every mode."""
    cache = {}
    for M, als in ((1, (2, 4)), (3, (2, 4)), (5, (4,))):
        cases = [("plain", D.plain_case("randn", "norm_R", M, K)) for K in (2560, 11008)]
        cases.append(("swiglu", D.swiglu_case("randn", M, 2560, 40)))
        cases.append(("qkv", D.qkv_case("randn", M, 2560, 64, 2, 1, True)))
        for name, c in cases:
            Wd, wa = weights_of(cache, c["W"], form)

            def once():
                if name == "plain":
                    return run_plain(c, Wd, wa)
                if name == "swiglu":
                    return ops.dec_proj(c["A"].to(BF).cuda(), Wd, **dev_args(c), **wa).double().cpu()
                return run_qkv(c, Wd, wa)[0]
            base = once()
            for al in als:
                with ops.L.knob("DEC_AL", al):
                    assert torch.equal(once(), base), (name, M, al)


# ------------------------------------------------------------------------------------------------ mode 1
@pytest.mark.parametrize("form", D.FORMS)
@pytest.mark.parametrize("K", D.SWIGLU_K)
@pytest.mark.parametrize("F", D.SWIGLU_F)
def test_swiglu(dev, F, K, form):
    """silu(gate) * up with the norm folded.  F = 40: a grid of 5 workgroups of 8 columns.  randn: gate pre-activations up to +-20 (the range of
    __expf matters: silu_bar grows with |gate|).  locate: every gate column is the same constant, up a distinct grid value per column, so a
    column that multiplies another column's up, or its own gate with up exchanged, is a wrong number; its accumulator carries the bar 0."""
    cache, worst = {}, [0.0, 0.0]
    for cid, c, exact in D.swiglu_cases(F, K):
        Wd, wa = weights_of(cache, c["W"], form)
        got = ops.dec_proj(c["A"].to(BF).cuda(), Wd, **dev_args(c), **wa).double().cpu()
        ref = D.dec_proj64(**c)
        if cid.startswith("randn"):
            assert 10.0 <= float(ref.z[:, :F].abs().max()) <= 40.0
        held(got, ref, exact, cid, worst)
    print(f"swiglu F={F} K={K} {form}: worst err/bar {worst[1]:.3e}")


# ------------------------------------------------------------------------------------------------ mode 2
@pytest.mark.parametrize("form", D.FORMS)
@pytest.mark.parametrize("K", D.QKV_K)
@pytest.mark.parametrize("heads,kvh", D.QKV_HEADS)
@pytest.mark.parametrize("hd", D.QKV_HD)
def test_qkv_real_angles(dev, hd, heads, kvh, K, form):
    """q | k | v with the norm folded and the table of position 1000 (cos and sin take all four sign pairs over the frequencies), adapters and bias
    off and on; the cache row is `pos` alone and pos + *pos_dev in turn, and every other cache row keeps its bytes."""
    cache, worst = {}, [0.0, 0.0]
    for i, (cid, c, exact) in enumerate(D.qkv_cases(hd, heads, kvh, K)):
        Wd, wa = weights_of(cache, c["W"], form)
        got, untouched = run_qkv(c, Wd, wa) if i % 2 == 0 else run_qkv(c, Wd, wa, pos=1, pos_dev=POS - 1)
        assert untouched, cid
        held(got, D.dec_proj64(**c), exact, cid, worst)
    print(f"qkv hd={hd} heads={heads}/{kvh} K={K} {form}: worst err/bar {worst[1]:.3e}")


@pytest.mark.parametrize("form", D.FORMS)
def test_position_outside_the_cache_writes_q_only(dev, form):
    """*pos_dev moves the row to exactly Tmax and to -1 (nothing farther out is tried): q is still right, and not one byte of the allocation
    the caches are cut from changes."""
    M, K, hd, heads, kvh = 5, 128, 32, 2, 1
    c = D.qkv_case("randn", M, K, hd, heads, kvh, True)
    wa = D.wargs(c["W"], form)
    Wd = wa.pop("W")
    ref = D.dec_proj64(**c)
    n = M * TMAX * c["dkv"]
    for pos, pos_dev in ((2, TMAX - 2), (0, -1)):
        big = torch.full((5 * n,), 123.0, dtype=BF, device=dev)
        kc, vc = big[n:2 * n].view(M, TMAX, -1), big[3 * n:4 * n].view(M, TMAX, -1)
        pd = torch.tensor([pos_dev], dtype=torch.int32, device=dev)
        q = ops.dec_proj(c["A"].to(BF).cuda(), Wd, rope=c["rope"].cuda(), kc=kc, vc=vc, pos=pos, pos_dev=pd, dq=c["dq"], dkv=c["dkv"], hd=hd,
                         **dev_args(c), **wa)
        assert bool((big == 123.0).all()), (pos, pos_dev)
        err = (q.double().cpu() - ref.out[:, :c["dq"]]).abs()
        assert bool((err <= bars.dec_proj_bar(ref)[:, :c["dq"]]).all()), (pos, pos_dev)


# ------------------------------------------------------------------------------------------------ strides and padding
@pytest.mark.parametrize("form", D.FORMS)
def test_strides_and_pad_columns(dev, form):
    """lda > K, ldc > N, ldr > N, ld_lora_t > 64 nmod, a 16-row C buffer for M = 5: the values are the packed launch's, every pad column of C
    and every row >= M keeps its canary."""
    M, K, N, r = 5, 384, D.N_PLAIN, 8
    c = D.plain_case("randn", "norm_R", M, K)
    c["out_f32"] = False
    lt = torch.zeros(M, 64)
    lt[:, :r] = torch.randn(M, r, generator=D.gen("slt"))
    lb = torch.zeros(N, 64)
    lb[:, :r] = torch.randn(N, r, generator=D.gen("slb")).to(BF).float()
    c.update(lt=lt, lbs=[lb], r=r, scale=0.25)
    wa = D.wargs(c["W"], form)
    Wd = wa.pop("W")
    ref = D.dec_proj64(**c)
    Abig = torch.full((M, K + 8), 9.0, dtype=BF, device=dev)
    Abig[:, :K] = c["A"].to(BF).cuda()
    Rbig = torch.full((M, N + 24), 5.0, dtype=BF, device=dev)
    Rbig[:, :N] = c["R"].to(BF).cuda()
    Tbig = torch.full((M, 72), 3.0, dtype=F32, device=dev)
    Tbig[:, :64] = lt.cuda()
    Cbig = torch.full((16, N + 16), 777.0, dtype=BF, device=dev)
    ops.dec_proj(Abig[:, :K], Wd, norm_w=c["g"].to(BF).cuda(), eps=c["eps"], R=Rbig[:, :N], out=Cbig[:M, :N], lora_t=Tbig[:, :64],
                 lora_b=[lb.to(BF).cuda()], lora_r=r, lora_scale=0.25, **wa)
    err = (Cbig[:M, :N].double().cpu() - ref.out).abs()
    assert bool((err <= bars.dec_proj_bar(ref)).all())
    assert bool((Cbig[:, N:] == 777.0).all()) and bool((Cbig[M:] == 777.0).all())
    # mode 2's q output with ldc > dq, adapters with ld_lora_t = 200 > 192 (qkv_case's own)
    cq = D.qkv_case("randn", M, K, 32, 2, 1, True)
    wq = D.wargs(cq["W"], form)
    Wq = wq.pop("W")
    Qbig = torch.full((16, cq["dq"] + 8), 777.0, dtype=BF, device=dev)
    kc = torch.zeros(M, TMAX, cq["dkv"], dtype=BF, device=dev)
    vc = torch.zeros_like(kc)
    ops.dec_proj(cq["A"].to(BF).cuda(), Wq, rope=cq["rope"].cuda(), kc=kc, vc=vc, pos=POS, dq=cq["dq"], dkv=cq["dkv"], hd=32, out=Qbig[:M, :cq["dq"]],
                 **dev_args(cq), **wq)
    rq = D.dec_proj64(**cq)
    got = torch.cat([Qbig[:M, :cq["dq"]], kc[:, POS], vc[:, POS]], 1).double().cpu()
    assert bool(((got - rq.out).abs() <= bars.dec_proj_bar(rq)).all())
    assert bool((Qbig[:, cq["dq"]:] == 777.0).all()) and bool((Qbig[M:] == 777.0).all())


# ------------------------------------------------------------------------------------------------ head dims the rotary index cannot serve
@pytest.mark.parametrize("hd", [48, 96])
def test_head_dim_not_a_power_of_two_is_refused(dev, hd):
    """The kernel's rotary index is (col % hd) & (hd / 2 - 1), which is col % (hd / 2) only for a power of two (hd = 96: column 16 would take
    angle 0): mode 2 refuses every other head dim instead of returning wrong rotations."""
    M, K, heads, kvh = 4, 128, 2, 1
    c = D.qkv_case("randn", M, K, hd, heads, kvh, False)
    kc = torch.zeros(M, TMAX, c["dkv"], dtype=BF, device=dev)
    with pytest.raises(ValueError, match="power of two"):
        ops.dec_proj(c["A"].to(BF).cuda(), c["W"].to(BF).cuda(), rope=c["rope"].cuda(), kc=kc, vc=torch.zeros_like(kc), pos=0, dq=c["dq"], dkv=c["dkv"],
                     hd=hd, **dev_args(c))
