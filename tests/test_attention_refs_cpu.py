"""CPU: the float64 attention restatements of tests/refs64_attention.py are right, and the attention bars of tests/bars.py have teeth.

  * attn_fwd64 / attn_bwd64 against torch's float64 scaled_dot_product_attention + autograd, 1e-12 relative (GQA, Tq != Tk causal, and the
    inverse-RoPE tail against refs64.rope).
  * Reachable: for every family and every geometry of the GPU file's table, the host emulation of the documented kernel arithmetic stays under
    every bar at every element (ratio < 1; the largest is printed).
  * Teeth: each mutant of the float64 reference -- the slips attention kernels make -- breaks at least one bar on at least one family.  The
    mutants are held to the bf16 bars, the widest there are."""
import pytest
import torch
import torch.nn.functional as F

import bars as Bar
import refs64 as R
import refs64_attention as A

F64 = torch.float64


def _sdpa(q, k, v, B, Tq, Tk, H, Hkv, hd, causal):
    q4 = q.double().reshape(B, Tq, H, hd).transpose(1, 2)
    k4 = k.double().reshape(B, Tk, Hkv, hd).transpose(1, 2).repeat_interleave(H // Hkv, 1)
    v4 = v.double().reshape(B, Tk, Hkv, hd).transpose(1, 2).repeat_interleave(H // Hkv, 1)
    mask = A.visible(Tq, Tk, causal)
    return F.scaled_dot_product_attention(q4, k4, v4, attn_mask=mask).transpose(1, 2).reshape(B * Tq, H * hd)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("B,Tq,Tk,H,Hkv,hd,causal", [(2, 37, 37, 4, 4, 16, True), (2, 37, 37, 4, 2, 16, False), (1, 20, 50, 8, 2, 8, True),
                                                      (2, 1, 33, 2, 1, 32, True), (2, 50, 197, 2, 2, 16, False)])
def test_fwd64_bwd64_against_torch(B, Tq, Tk, H, Hkv, hd, causal):
    q, k, v, dout = (t.double() for t in A.make_inputs("randn", B, Tq, Tk, H, Hkv, hd, causal))
    scale = hd ** -0.5
    o, lse, p = A.attn_fwd64(q, k, v, B, Tq, Tk, H, Hkv, hd, causal, scale)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    ref = _sdpa(qg, kg, vg, B, Tq, Tk, H, Hkv, hd, causal)
    assert _rel(o, ref.detach()) < 1e-12
    s = torch.einsum("bhid,bhjd->bhij", A._heads(q, B, Tq, H, hd, F64), A._heads(k, B, Tk, Hkv, hd, F64)[:, A.head_map(H, Hkv)]) * scale
    s = s.masked_fill(~A.visible(Tq, Tk, causal), float("-inf"))
    assert _rel(lse, torch.logsumexp(s, -1)) < 1e-12 and _rel(p, torch.softmax(s, -1)) < 1e-12
    if Tq == Tk:
        ref.backward(dout)
        dq, dk, dv = A.attn_bwd64(q, k, v, dout, B, Tq, H, Hkv, hd, causal, scale)
        assert _rel(dq, qg.grad) < 1e-12 and _rel(dk, kg.grad) < 1e-12 and _rel(dv, vg.grad) < 1e-12


def test_bwd64_rope_tail_against_refs64_rope():
    """The gradient with respect to the pre-RoPE q, k is the transpose rotation of the gradient with respect to the rotated ones: autograd through
    SDPA on the rotated q, k, then refs64.rope(inverse=True), == attn_bwd64 with the rotary tail."""
    B, T, H, Hkv, hd, pos0, theta = 2, 19, 4, 2, 16, 5, 10000.0
    q, k, v, dout = (t.double() for t in A.make_inputs("randn", B, T, T, H, Hkv, hd, True))
    pos = torch.arange(pos0, pos0 + T)
    qr, kr = R.rope(q, T, H, hd, pos, theta).requires_grad_(True), R.rope(k, T, Hkv, hd, pos, theta).requires_grad_(True)
    _sdpa(qr, kr, v, B, T, T, H, Hkv, hd, True).backward(dout)
    want_dq, want_dk = R.rope(qr.grad, T, H, hd, pos, theta, inverse=True), R.rope(kr.grad, T, Hkv, hd, pos, theta, inverse=True)
    ang = R.rope_angles(pos, hd, theta).to(F64)
    dq, dk, _ = A.attn_bwd64(qr.detach(), kr.detach(), v, dout, B, T, H, Hkv, hd, True, hd ** -0.5, rope=(ang.cos(), ang.sin()))
    assert _rel(dq, want_dq) < 1e-12 and _rel(dk, want_dk) < 1e-12


def _ratio(x, ref, bar):
    err = (x.double() - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    bar = bar if torch.is_tensor(bar) else torch.tensor(float(bar), dtype=F64)
    return float((err / bar).max())


@pytest.mark.parametrize("g", A.GEOMETRIES, ids=A.geo_id)
def test_emulation_stays_under_every_bar(g):
    worst = {}
    for fam in A.FAMILIES:
        c = A.case(g, fam)
        r = {"o": _ratio(c.emul["o"], c.o64, c.bar_o), "lse": _ratio(c.emul["lse"], c.lse64, c.bar_lse)}
        if A.has_bwd(g):
            for n in ("dq", "dk", "dv"):
                r[n] = A.bwd_ratio(c, g, n, c.emul_b[n])                 # the whole tensor and every head slice against its own bar
                rl2 = getattr(c, "rel_l2_" + n)
                if rl2 is not None:
                    r[n + "-rel_l2"] = Bar.rel_l2(c.emul_b[n].double(), getattr(c, n + "64")) / rl2
                if fam == "count":
                    r["count-" + n] = _ratio(c.emul_b[n], getattr(c, n + "64"), getattr(c, "ebar_" + n))
        for kk, vv in r.items():
            assert vv < 1.0, f"{A.geo_id(g)} {fam} {kk}: the emulation is at {vv:.3f} of its bar"
            worst[kk] = max(worst.get(kk, 0.0), vv)
    print(A.geo_id(g), {kk: round(vv, 3) for kk, vv in worst.items()})


# ---------------------------------------------------------------- mutants
def _bf16_geo(form):
    return [g for g in A.GEOMETRIES if g.dt == "bf16" and g.form == form]


def _broken_fwd(c, o, lse):
    return _ratio(o, c.o64, c.bar_o) > 1.0 or _ratio(lse, c.lse64, c.bar_lse) > 1.0


def _fwd_mutant(g, fam, mutant):
    c = A.case(g, fam)
    B, Tq, Tk, H, Hkv, hd = g.B, g.Tq, g.Tk, g.H, g.Hkv, g.hd
    k, v, vis, hmap, Tk2 = c.k, c.v, A.visible(Tq, Tk, g.causal), None, Tk
    if mutant == "zero_key_past_Tk":                         # one zero-padded key (and value) row past Tk that every query sees
        pad = (lambda x: torch.cat([x.reshape(B, Tk, -1), torch.zeros(B, 1, x.shape[1], dtype=x.dtype)], 1).reshape(B * (Tk + 1), -1))
        k, v, Tk2 = pad(k), pad(v), Tk + 1
        vis = torch.cat([vis, torch.ones(Tq, 1, dtype=torch.bool)], 1)
    elif mutant == "last_key_dropped":
        vis = vis.clone()
        vis[:, Tk - 1] = False
    elif mutant in ("causal_edge+1", "causal_edge-1"):
        vis = A.visible(Tq, Tk, True, shift=1 if mutant.endswith("+1") else -1)
    elif mutant == "neighbour_kv_head":                      # the last query head of group 0 reads kv head 1
        hmap = A.head_map(H, Hkv).clone()
        hmap[H // Hkv - 1] = 1
    o, lse, _ = A.attn_fwd64(c.q, k, v, B, Tq, Tk2, H, Hkv, hd, g.causal, c.scale, vis=vis, hmap=hmap)
    return _broken_fwd(c, o, lse)


FWD_MUTANTS = {
    "zero_key_past_Tk": [g for g in A.GEOMETRIES if g.dt == "bf16" and g.form in ("short13x7", "mfma64x4", "mfma128x4", "tqtk-mfma64x4") and g.Tk > 1],
    "last_key_dropped": [g for g in A.GEOMETRIES if g.dt == "bf16" and g.form in ("short13x7", "short17x9", "mfma64x4", "mfma128x4") and g.Tk > 1],
    "causal_edge+1": [g for g in A.GEOMETRIES if g.dt == "bf16" and g.causal and g.Tk > 1 and g.form != "ref"],
    "causal_edge-1": [g for g in A.GEOMETRIES if g.dt == "bf16" and g.causal and g.Tk > 1 and g.form != "ref"],
    "neighbour_kv_head": [g for g in A.GEOMETRIES if g.dt == "bf16" and g.Hkv > 1 and g.H > g.Hkv],
}


@pytest.mark.parametrize("mutant", list(FWD_MUTANTS))
def test_forward_mutants_break_a_bar(mutant):
    """On EVERY geometry where the slip can happen at least one family catches it (and the count family always does)."""
    for g in FWD_MUTANTS[mutant]:
        if mutant == "causal_edge+1" and g.Tq == 1:          # the one query already sees every key
            continue
        caught = [fam for fam in A.FAMILIES if _fwd_mutant(g, fam, mutant)]
        print(mutant, A.geo_id(g), "caught by", caught)
        assert caught, f"{mutant} passes every bar on {A.geo_id(g)}"
        assert "count" in caught, f"{mutant} on {A.geo_id(g)}: the count family missed it"


def _bwd_mutant(g, fam, mutant):
    c = A.case(g, fam)
    T = g.Tq
    kw, rope = {}, None
    if mutant == "delta_left_out":
        kw["use_delta"] = False
    elif mutant == "dk_misses_row_31_of_32":
        kw["dk_rows"] = torch.arange(T) % 32 != 31
    dq, dk, dv = A.attn_bwd64(c.bq, c.bk, c.bv, c.bdout, g.B, T, g.H, g.Hkv, g.hd, g.causal, c.scale, **kw)
    bad = False
    for n, x in (("dq", dq), ("dk", dk), ("dv", dv)):
        bad |= A.bwd_ratio(c, g, n, x) > 1.0
        rl2 = getattr(c, "rel_l2_" + n)
        if rl2 is not None:
            bad |= Bar.rel_l2(x, getattr(c, n + "64")) > rl2
        if fam == "count":
            bad |= _ratio(x, getattr(c, n + "64"), getattr(c, "ebar_" + n)) > 1.0
    return bad


BWD_GEO = [g for g in A.GEOMETRIES if g.dt == "bf16" and A.has_bwd(g) and g.Tq >= 32 and g.form in ("short13x7", "mfma64x4", "mfma128x4", "gqa-mfma128x4")]


@pytest.mark.parametrize("mutant", ["delta_left_out", "dk_misses_row_31_of_32"])
def test_backward_mutants_break_a_bar(mutant):
    for g in BWD_GEO:
        caught = [fam for fam in A.FAMILIES if _bwd_mutant(g, fam, mutant)]
        print(mutant, A.geo_id(g), "caught by", caught)
        assert caught, f"{mutant} passes every bar on {A.geo_id(g)}"


def test_rope_applied_forward_breaks_a_bar():
    g = A._g("rope-bwd-mfma128x4", 70, 128, True, "mfma", H=4, Hkv=2)
    ang = R.rope_angles(torch.arange(5, 75), g.hd, 10000.0).to(F64)
    rope = (ang.cos().float().double(), ang.sin().float().double())
    c = A.case(g, "randn", rope=rope, rope_key="cpu5")
    for n in ("dq", "dk", "dv"):
        assert A.bwd_ratio(c, g, n, c.emul_b[n]) < 1.0
    dq, dk, _ = A.attn_bwd64(c.bq, c.bk, c.bv, c.bdout, g.B, g.Tq, g.H, g.Hkv, g.hd, True, c.scale, rope=rope, rope_forward=True)
    assert A.bwd_ratio(c, g, "dq", dq) > 1.0 and A.bwd_ratio(c, g, "dk", dk) > 1.0
