"""What tests/test_decode_pin_gpu.py rests on, checked without a GPU: the float64 restatement of avllm_dec_proj against plain torch composed
from refs64 (and transformers' apply_rotary_pos_emb where it is installed); the host emulation of the kernel's fp32 arithmetic under the
derived bar on the very cases the GPU file runs, with the premises of the `exact` and `locate` families; every mutant of the emulation over
the bar in the family meant to catch it; and the K values of the GPU file reaching every tail of every ring depth."""
import pytest
import torch

import bars
import refs64
import refs64_decode as D

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16


def over(ref, out, exact=False):
    """Worst err / bar of an emulated output (0 / 0 counts as 0; x / 0 as inf)."""
    err = (out - ref.out).abs()
    bar = bars.dec_proj_bar(ref, exact=exact)
    if exact and ref.rstd is None and ref.out_f32:
        bar = torch.zeros_like(bar)
    return float(torch.where(err == 0, torch.zeros_like(err), err / bar.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------ the restatement against plain torch
def test_restatement_is_plain_torch_float64():
    M, K, N, r = 5, 256, 48, 8
    A = D.acts("randn", M, K, "pin")
    W = torch.randn(N, K, generator=D.gen("pw")).to(BF).float()
    g = D.rand_norm(K, "pin")
    R = torch.randn(M, N, generator=D.gen("pr")).to(BF).float()
    b = torch.randn(N, generator=D.gen("pb")).to(BF).float()
    lt = torch.randn(M, 64, generator=D.gen("plt"))
    lb = torch.randn(N, 64, generator=D.gen("plb")).to(BF).float()
    # the fold rounds x g to bf16 BEFORE the rstd: compose rmsnorm_fwd on that rounded product with unit weights
    xg = (A * g).to(BF).double()
    rstd = refs64.rmsnorm_fwd(A, torch.ones(K), 1e-5)[1][:, None]
    z = (xg @ W.double().t()) * rstd + b.double() + 0.5 * (lt[:, :r].double() @ lb[:, :r].double().t())
    ref = D.dec_proj64(A, W, g=g, eps=1e-5, R=R, bias=b, lt=lt, lbs=[lb], r=r, scale=0.5, out_f32=True)
    assert torch.allclose(ref.out, z + R.double(), rtol=1e-13, atol=1e-13)
    assert torch.equal(ref.rounded, ref.out.float().double())
    # without the bf16 rounding of the fold (g = 1) it IS rmsnorm_fwd followed by the product
    y1 = refs64.rmsnorm_fwd(A, torch.ones(K), 1e-5)[0] @ W.double().t()
    assert torch.allclose(D.dec_proj64(A, W, g=torch.ones(K), eps=1e-5, out_f32=True).out, y1, rtol=1e-12, atol=1e-13)
    # SwiGLU
    ref = D.dec_proj64(A, W, mode=D.SWIGLU, g=g, eps=1e-5)
    assert torch.allclose(ref.out, refs64.swiglu_fwd((xg @ W.double().t()) * rstd), rtol=1e-13, atol=1e-13)
    assert torch.equal(ref.rounded, ref.out.float().to(BF).double())
    # q | k | v with real angles: refs64.rope at the same position (float64 table of HF's fp32 angle)
    hd, heads, kvh, pos, theta = 32, 2, 1, D.ROPE_POS, 10000.0
    dq, dkv = heads * hd, kvh * hd
    Wq = torch.randn(dq + 2 * dkv, K, generator=D.gen("pq")).to(BF).float()
    ang = refs64.rope_angles([pos], hd, theta)[0].double()
    tab64 = torch.stack([ang.cos(), ang.sin()], -1)
    assert torch.equal(tab64.float(), D.real_rope(hd, pos, theta))
    ref = D.dec_proj64(A, Wq, mode=D.QKV, g=g, eps=1e-5, dq=dq, dkv=dkv, hd=hd, rope=tab64)
    zq = (xg @ Wq.double().t()) * rstd
    want = torch.cat([refs64.rope(zq[:, :dq], 1, heads, hd, [pos], theta), refs64.rope(zq[:, dq:dq + dkv], 1, kvh, hd, [pos], theta), zq[:, dq + dkv:]], 1)
    assert torch.allclose(ref.out, want, rtol=1e-13, atol=1e-13)
    # the bias-test helper `rot` is the same rotation for one angle
    one = D.dec_proj64(A, Wq, mode=D.QKV, dq=dq, dkv=dkv, hd=hd, rope=torch.tensor([[0.6, 0.8]], dtype=F64).repeat(hd // 2, 1))
    assert torch.allclose(one.out[:, :dq], D.rot(one.z[:, :dq].clone(), heads, hd, 0.6, 0.8), rtol=1e-13, atol=1e-13)


def test_rotation_is_transformers_apply_rotary_pos_emb():
    """Pairs (i, i + hd/2), signs and the table's layout against HF's own function (float64 in, float64 out); the issue's fallback when
    transformers lacks it is refs64.rope, which the test above holds in any case."""
    try:
        from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    except ImportError:
        def apply_rotary_pos_emb(q, k, cos, sin):                      # no transformers here: refs64.rope's rotate-half, the pin the issue names for that case
            def rh(x):
                return torch.cat([-x[..., x.shape[-1] // 2:], x[..., : x.shape[-1] // 2]], -1)
            return q * cos.unsqueeze(1) + rh(q) * sin.unsqueeze(1), k * cos.unsqueeze(1) + rh(k) * sin.unsqueeze(1)
    M, K = 4, 128
    for hd, heads, kvh in ((32, 4, 2), (64, 3, 3), (128, 2, 1)):
        dq, dkv = heads * hd, kvh * hd
        c = D.qkv_case("randn", M, K, hd, heads, kvh, False)
        ref = D.dec_proj64(**c)
        tab = c["rope"].double()
        cos, sin = torch.cat([tab[:, 0], tab[:, 0]])[None, None, :], torch.cat([tab[:, 1], tab[:, 1]])[None, None, :]      # [batch, seq = 1, hd]
        q = ref.z[:, :dq].reshape(M, heads, 1, hd)
        k = ref.z[:, dq:dq + dkv].reshape(M, kvh, 1, hd)
        qe, ke = apply_rotary_pos_emb(q, k, cos, sin)
        assert torch.allclose(ref.out[:, :dq], qe.reshape(M, dq), rtol=1e-14, atol=1e-14)
        assert torch.allclose(ref.out[:, dq:dq + dkv], ke.reshape(M, dkv), rtol=1e-14, atol=1e-14)
        assert torch.equal(ref.out[:, dq + dkv:], ref.z[:, dq + dkv:])


def test_helper_weights_are_held_by_every_form_and_differ_where_a_slip_looks():
    for form in D.FORMS:
        for K in (128, 384, 11008):
            assert D.holds(D.grid_weights(D.N_PLAIN, K), form) and D.holds(D.locate_weights(D.N_PLAIN, K), form)
            assert D.holds(D.mx_weights(16, K, "h"), form)
        for W in (D.grid_weights(D.N_PLAIN, 384), D.locate_weights(D.N_PLAIN, 384)):
            e = D.block_exponents(W, form)
            if e is not None:
                assert bool((e[:, 1:] != e[:, :-1]).all()), form                       # neighbouring blocks: distinct exponent bytes, fp8 too
    W = D.locate_weights(D.N_PLAIN, 512)
    k = torch.arange(512)
    for d in (1, 2, 4):                                                                # the 8 elements of a lane's step: a swapped nibble, byte, dword
        assert bool((W[:, k] != W[:, k ^ d]).all())
    for d in (8, 16, 24, 32, 64, 96):                                                  # the other steps of a lane, in every form
        kk = k[:-d]
        assert bool((W[:, kk] != W[:, kk + d]).all())
    n = torch.arange(D.N_PLAIN)
    assert bool((W[n] != W[n ^ 8]).all()) and bool((W[:-1] != W[1:]).all()) and bool((W[:-16] != W[16:]).all())
    g = D.step_norm(512)
    for form in D.FORMS:
        for j in range(4):
            assert bool((g[torch.from_numpy(D.step_cols(form, j))] != g[torch.from_numpy(D.step_cols(form, (j + 1) % 4))]).all())


# ------------------------------------------------------------------------------------------------ the ring: every tail of every depth
def test_k_values_reach_every_tail_of_every_ring_depth():
    """From the deal formula and the depth table: over K_DEAL the 8 waves hold 0 .. 11 groups, so the straight-line tails 1 .. 2 D - 1 of D = 2
    (bf16, fp8), D = 3 (fp4, M > 8) and D = 4 (fp4, M <= 8) all run, and each tail >= D (the only ones a trip of the main loop can precede: the
    loop leaves D <= rem < 2 D groups) runs both after a trip and without one."""
    groups = {G for K in D.K_DEAL for _, G in D.deal(K)}
    assert groups == set(range(12))
    for K in D.K_DEAL:
        dl = D.deal(K)
        assert sum(G for _, G in dl) == K // 128 and all(dl[w][0] + 128 * dl[w][1] == dl[w + 1][0] for w in range(7)) and dl[0][0] == 0
    seen = {}
    for form in D.FORMS:
        for M in D.M_DEAL:
            Dp = D.depth(form, D.al_of(M))
            for G in groups:
                trips, rem = D.ring_path(G, Dp)
                seen.setdefault(Dp, set()).add((trips > 0, rem))
    assert set(seen) == {2, 3, 4}
    for Dp, paths in seen.items():
        for T in range(1, 2 * Dp):
            assert (False, T) in paths, (Dp, T)
            if T >= Dp:
                assert (True, T) in paths, (Dp, T)
    assert {D.al_of(M) for M in D.M_DEAL} == {1, 2, 4} and [D.al_of(M) for M in D.M_DEAL] == [1, 1, 2, 2, 4, 4]


# ------------------------------------------------------------------------------------------------ the emulation under the bar, on the GPU file's cases
@pytest.mark.parametrize("form", D.FORMS)
@pytest.mark.parametrize("K", D.K_DEAL)
def test_emulation_is_under_the_bar_plain(K, form):
    worst = 0.0
    for cid, c, exact in D.plain_cases(K):
        assert D.holds(c["W"], form)
        ref = D.dec_proj64(**c)
        if exact:
            assert D.premise_exact(ref), cid                                           # sums below 2^24 units of 2^-4
            if c.get("R") is not None and c.get("g") is None:
                assert torch.equal(ref.out, ref.rounded)
        r = over(ref, D.emul(form=form, **c), exact)
        worst = max(worst, r)
        assert r <= 1.0, (cid, r)
    print(f"emul plain K={K} {form}: worst err/bar {worst:.3e}")


@pytest.mark.parametrize("form", D.FORMS)
@pytest.mark.parametrize("K", D.K_DEAL)
def test_emulation_passes_locate(K, form):
    """The locate walk over the emulation at M = 16, and at M = 5 too for K <= 384 (the other row counts are the same construction with more
    launches, and the emulation takes a second per hundred of them; the GPU file runs all six at every K): the premise is that every expected
    value is one weight times a power of two, representable in fp32, and locate_weights is held by the form."""
    W = D.locate_weights(D.N_PLAIN, K)
    assert D.holds(W, form)
    g = D.step_norm(K)

    def run(A, norm):
        return torch.stack([D.emul(A[l], W, form, g=g if norm else None, eps=D.EPS, out_f32=True) for l in range(A.shape[0])])
    D.locate_check(run, K, Ms=(5, 16) if K <= 384 else (16,))


@pytest.mark.parametrize("form", D.FORMS)
def test_emulation_is_under_the_bar_swiglu_and_qkv(form):
    worst = {"swiglu": 0.0, "qkv": 0.0}
    for F in D.SWIGLU_F:
        for K in D.SWIGLU_K:
            for cid, c, exact in D.swiglu_cases(F, K):
                assert D.holds(c["W"], form)
                ref = D.dec_proj64(**c)
                if exact:
                    assert torch.equal(ref.acc, ref.acc.float().double())              # one product per sum: representable
                r = over(ref, D.emul(form=form, **c), exact)
                worst["swiglu"] = max(worst["swiglu"], r)
                assert r <= 1.0, ("swiglu", F, K, cid, r)
    for hd in D.QKV_HD:
        for heads, kvh in D.QKV_HEADS:
            for K in D.QKV_K:
                for cid, c, exact in D.qkv_cases(hd, heads, kvh, K):
                    ref = D.dec_proj64(**c)
                    r = over(ref, D.emul(form=form, **c), exact)
                    worst["qkv"] = max(worst["qkv"], r)
                    assert r <= 1.0, ("qkv", hd, heads, kvh, K, cid, r)
    print(f"emul {form}: worst err/bar {worst}")


# ------------------------------------------------------------------------------------------------ every mutant is caught
def _plain(fam, variant, M, K):
    return D.plain_case(fam, variant, M, K), fam == "exact"


def _locate(form, M, K, norm):
    """The locate walk as a mutant sees it: (case-like runner) -> True when locate_check raises."""
    W, g = D.locate_weights(D.N_PLAIN, K), D.step_norm(K)

    def caught(mutant):
        def run(A, nrm):
            return torch.stack([D.emul(A[l], W, form, g=g if nrm else None, eps=D.EPS, out_f32=True, mutant=mutant) for l in range(A.shape[0])])
        try:
            D.locate_check(run, K, Ms=(M,))
        except AssertionError:
            return True
        return False
    return caught


# mutant -> the cases of the GPU file's lists meant to catch it: (family, builder); FORM_OF names the weight form each is emulated in
CATCHERS = {
    "drop_last_group": [("exact", lambda: _plain("exact", "plain", 5, 2560)), ("exact", lambda: _plain("exact", "plain", 16, 11008))],
    "k0_overlap": [("exact", lambda: _plain("exact", "plain", 8, 384)), ("exact", lambda: _plain("exact", "plain", 1, 6656))],
    "exp_neighbour": [("exact", lambda: _plain("exact", "plain", 4, 128)), ("exact", lambda: _plain("exact", "plain", 9, 4608))],
    "nibble_swap": [("exact", lambda: _plain("exact", "plain", 1, 128))],
    "norm_next_step": [("exact", lambda: _plain("exact", "norm", 5, 384))] * 3,
    "al_rotate": [("exact", lambda: _plain("exact", "plain", 9, 128)), ("exact", lambda: _plain("exact", "plain", 16, 2560))],
    "rstd_before_round": [("exact", lambda: _plain("exact", "norm", 5, 128)), ("randn", lambda: _plain("randn", "norm", 16, 128))],
    "r_after_round": [("offset", lambda: _plain("offset", "norm_R", 5, 2560)), ("offset", lambda: _plain("offset", "norm_R", 16, 128))],
    "gate_up_swapped": [("swiglu randn", lambda: (D.swiglu_case("randn", 8, 128, 8), False)),
                        ("swiglu locate", lambda: (D.swiglu_case("locate", 1, 2560, 40), True))],
    "rot_sign_flip": [("qkv", lambda: (D.qkv_case("randn", 5, 128, 32, 3, 3, False), False))],
    "bias_after_rot": [("qkv", lambda: (D.qkv_case("randn", 5, 128, 64, 2, 1, True, True), False))],
    "lora_after_rot": [("qkv", lambda: (D.qkv_case("randn", 1, 128, 32, 4, 2, True, False), False))],
    "bias_lora_after_rot": [("qkv", lambda: (D.qkv_case("randn", 16, 2560, 128, 2, 1, True, True), False))],
    "lora_module_off": [("qkv", lambda: (D.qkv_case("randn", 5, 128, 64, 3, 3, True, False), False))],
    # the kernel's own index expression: right at every power of two, wrong at hd = 96, which is why the host check refuses it.  No GPU case can
    # show it (the launch is refused); the restatement at hd = 96 does.
    "rot_index_mask": [("qkv hd=96, host only", lambda: (D.qkv_case("randn", 4, 128, 96, 2, 1, False), False))],
}
FORM_OF = {"drop_last_group": ("bf16", "fp4"), "k0_overlap": ("fp8", "bf16"), "exp_neighbour": ("fp8", "fp4"), "nibble_swap": ("fp4",),
           "norm_next_step": D.FORMS, "al_rotate": ("bf16", "fp4"), "rstd_before_round": ("bf16", "fp8"), "r_after_round": ("bf16", "fp4"),
           "gate_up_swapped": ("bf16", "fp4"), "rot_sign_flip": ("bf16",), "bias_after_rot": ("fp8",), "lora_after_rot": ("bf16",),
           "bias_lora_after_rot": ("fp4",), "lora_module_off": ("bf16",), "rot_index_mask": ("bf16",)}


@pytest.mark.parametrize("mutant", D.MUTANTS)
def test_every_mutant_is_over_the_bar(mutant):
    """Each slip of the emulation exceeds the bar in EVERY case listed for it (all of them cases of the GPU file's lists, but the hd = 96 one), while
    the unmutated emulation passes the same case: the tests can see it."""
    assert set(CATCHERS) == set(D.MUTANTS)
    for (fam, build), form in zip(CATCHERS[mutant], FORM_OF[mutant]):
        c, exact = build()
        ref = D.dec_proj64(**c)
        clean, bad = over(ref, D.emul(form=form, **c), exact), over(ref, D.emul(form=form, mutant=mutant, **c), exact)
        print(f"{mutant}: {fam} {form} M={c['A'].shape[0]} K={c['A'].shape[1]}: err/bar {bad:.3e} (unmutated {clean:.3e})")
        assert clean <= 1.0 < bad, (mutant, fam, form, clean, bad)


@pytest.mark.parametrize("mutant,form,M,K", [("nibble_swap", "fp4", 16, 384), ("exp_neighbour", "fp8", 5, 384), ("exp_neighbour", "fp4", 16, 128),
                                             ("norm_next_step", "bf16", 16, 128), ("norm_next_step", "fp8", 5, 384), ("norm_next_step", "fp4", 16, 128),
                                             ("drop_last_group", "bf16", 16, 384), ("al_rotate", "fp8", 16, 128)])
def test_locate_catches_the_index_mutants(mutant, form, M, K):
    caught = _locate(form, M, K, True)
    assert not caught(None) and caught(mutant)


def test_head_dim_96_is_where_the_mask_goes_wrong():
    """(col % hd) & (hd / 2 - 1) against col % (hd / 2): equal for every power of two from 32 up, different at 48, 80, 96, 112 (hd = 96: column 16
    takes index 0)."""
    for hd in (32, 64, 128, 256):
        i = torch.arange(hd)
        assert torch.equal(i & (hd // 2 - 1), i % (hd // 2))
    for hd in (48, 80, 96, 112):
        i = torch.arange(hd)
        assert not torch.equal(i & (hd // 2 - 1), i % (hd // 2))
    assert (16 % 96) & (96 // 2 - 1) == 0
