"""Plain float64 restatements of softmax attention, forward and backward (csrc/attention.hip, attention_bwd.hip, attention_ref.hip), a host
emulation of the arithmetic those files document, the deterministic input families and the geometry table of tests/test_attention_pin_gpu.py.

No fused torch op is used: scores, mask, max, exp, sum, division and every product of the backward are written out.  Every function takes the
operands as the kernel sees them (q [B*Tq, H*hd], k / v [B*Tk, Hkv*hd], row = token, head h at column h*hd; bf16 tensors are upcast, never
re-drawn) and computes in `dtype`: float64 is the reference, float32 the host measurement tests/bars.py derives the fp32 bars from.
tests/test_attention_refs_cpu.py pins attn_fwd64 / attn_bwd64 to torch's float64 scaled_dot_product_attention + autograd and shows that the
bars of tests/bars.py separate attn_emul from the mutants it builds out of the hooks of _fwd_core / _bwd_core.  Nothing here touches the GPU."""
import math
from collections import namedtuple

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
LOG2E_F32 = 1.4426950408889634          # the kernels multiply by this literal in fp32
LN2_F32 = 0.69314718055994531


def _c(t, dtype):
    return None if t is None else t.detach().to("cpu").to(dtype)


def _heads(x, B, T, H, hd, dtype):
    """[B*T, H*hd] -> [B, H, T, hd]"""
    return _c(x, dtype).reshape(B, T, H, hd).permute(0, 2, 1, 3)


def _rows(x4):
    """[B, H, T, hd] -> [B*T, H*hd]"""
    B, H, T, hd = x4.shape
    return x4.permute(0, 2, 1, 3).reshape(B * T, H * hd)


def visible(Tq, Tk, causal, shift=0):
    """[Tq, Tk] bool: causal query t sees keys <= t + (Tk - Tq) (+ shift: the mutants' off-by-one edge)."""
    if not causal:
        return torch.ones(Tq, Tk, dtype=torch.bool)
    return torch.arange(Tk)[None, :] <= torch.arange(Tq)[:, None] + (Tk - Tq) + shift


def head_map(H, Hkv):
    """query head h reads key/value head h // (H / Hkv) (HF repeat_kv)."""
    return torch.arange(H) // (H // Hkv)


def _fwd_core(q4, k4, v4, vis, scale):
    """q4 [B,H,Tq,hd], k4 / v4 [B,H,Tk,hd] (already expanded to query heads), vis [Tq,Tk] -> o4, lse [B,H,Tq], w [B,H,Tq,Tk]."""
    s = torch.einsum("bhid,bhjd->bhij", q4, k4) * scale
    s = s.masked_fill(~vis, float("-inf"))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    w = e / l
    return torch.einsum("bhij,bhjd->bhid", w, v4), (m + torch.log(l))[..., 0], w


def attn_fwd64(q, k, v, B, Tq, Tk, H, Hkv, hd, causal, scale, dtype=F64, vis=None, hmap=None):
    """-> (o [B*Tq, H*hd], lse [B,H,Tq] natural log, p [B,H,Tq,Tk] the softmax).  vis / hmap: the mutants' hooks (a visibility matrix and a
    query-head -> kv-head map other than the right ones)."""
    vis = visible(Tq, Tk, causal) if vis is None else vis
    hmap = head_map(H, Hkv) if hmap is None else hmap
    q4, k4, v4 = _heads(q, B, Tq, H, hd, dtype), _heads(k, B, Tk, Hkv, hd, dtype), _heads(v, B, Tk, Hkv, hd, dtype)
    o4, lse, w = _fwd_core(q4, k4[:, hmap], v4[:, hmap], vis, scale)
    return _rows(o4), lse, w


def unrope(x4, rope, forward=False):
    """The inverse rotary embedding (transpose of the rotate-half rotation) on [B, heads, T, hd] from rope = (cos, sin), each [T, hd/2]:
    (a, b) -> (a c + b s, b c - a s).  forward=True applies the rotation itself (a mutant)."""
    cos, sin = (t.to(x4.dtype)[None, None] for t in rope)
    if forward:
        sin = -sin
    hd = x4.shape[-1]
    a, b = x4[..., : hd // 2], x4[..., hd // 2:]
    return torch.cat([a * cos + b * sin, b * cos - a * sin], -1)


def _bwd_core(q4, k4, v4, do4, vis, scale, use_delta=True, dk_rows=None):
    """Autograd of _fwd_core written out -> dq4, dk4, dv4 per QUERY head (the caller sums groups).  use_delta / dk_rows: the mutants' hooks
    (delta left out of dS; a [Tq] bool of the query rows that reach dK)."""
    o4, _, w = _fwd_core(q4, k4, v4, vis, scale)
    dp = torch.einsum("bhid,bhjd->bhij", do4, v4)
    delta = (do4 * o4).sum(-1, keepdim=True)
    ds = w * (dp - delta if use_delta else dp) * scale
    dq4 = torch.einsum("bhij,bhjd->bhid", ds, k4)
    dsk = ds if dk_rows is None else ds * dk_rows.to(ds.dtype)[None, None, :, None]
    dk4 = torch.einsum("bhij,bhid->bhjd", dsk, q4)
    dv4 = torch.einsum("bhij,bhid->bhjd", w, do4)
    return dq4, dk4, dv4


def _group_sum(x4, Hkv):
    B, H, T, hd = x4.shape
    return x4.reshape(B, Hkv, H // Hkv, T, hd).sum(2)


def attn_bwd64(q, k, v, dout, B, T, H, Hkv, hd, causal, scale, rope=None, dtype=F64, vis=None, hmap=None, use_delta=True, dk_rows=None,
               rope_forward=False):
    """-> (dq [B*T, H*hd], dk, dv [B*T, Hkv*hd]): the gradient of sum(o * dout), dk / dv summed over the query heads of each group; with
    rope = (cos, sin) [T, hd/2] the inverse rotary is applied to dq and dk (the gradient with respect to the pre-RoPE q and k)."""
    vis = visible(T, T, causal) if vis is None else vis
    right_map = hmap is None
    hmap = head_map(H, Hkv) if hmap is None else hmap
    q4, k4, v4 = _heads(q, B, T, H, hd, dtype), _heads(k, B, T, Hkv, hd, dtype), _heads(v, B, T, Hkv, hd, dtype)
    do4 = _heads(dout, B, T, H, hd, dtype)
    dq4, dk4, dv4 = _bwd_core(q4, k4[:, hmap], v4[:, hmap], do4, vis, scale, use_delta, dk_rows)
    if right_map:
        dk4, dv4 = _group_sum(dk4, Hkv), _group_sum(dv4, Hkv)
    else:                                                     # a mutant's map: scatter every query head's share to the kv head it read
        zk, zv = torch.zeros_like(k4), torch.zeros_like(v4)
        dk4, dv4 = zk.index_add(1, hmap, dk4), zv.index_add(1, hmap, dv4)
    if rope is not None:
        dq4, dk4 = unrope(dq4, rope, rope_forward), unrope(dk4, rope, rope_forward)
    return _rows(dq4), _rows(dk4), _rows(dv4)


def delta_amplification(q, k, v, dout, B, T, H, Hkv, hd, causal, scale):
    """How much the ONE bf16 rounding of O that reaches delta = rowsum(dO * O) weighs in dS = P (dP - delta), relative to dS itself, pooled over
    rows: sqrt(sum_i sum_d (dO_id O_id)^2 / sum_i sum_j w_ij (dP_ij - delta_i)^2).  About 1 for centred V; mu / sigma for V = mu + sigma z (the
    `offset` family), and large where the softmax is one-hot and dS is a cancellation (`sharp`)."""
    q4, k4, v4 = _heads(q, B, T, H, hd, F64), _heads(k, B, T, Hkv, hd, F64), _heads(v, B, T, Hkv, hd, F64)
    do4 = _heads(dout, B, T, H, hd, F64)
    hm = head_map(H, Hkv)
    o4, _, w = _fwd_core(q4, k4[:, hm], v4[:, hm], visible(T, T, causal), scale)
    dp = torch.einsum("bhid,bhjd->bhij", do4, v4[:, hm])
    delta = (do4 * o4).sum(-1, keepdim=True)
    num = float(((do4 * o4) ** 2).sum())
    den = float((w * (dp - delta) ** 2).sum())
    return math.sqrt(num / max(den, 1e-300))


# ---------------------------------------------------------------- emulation of the documented kernel arithmetic
def _bf(x):
    return x.to(BF16).to(F32)


def attn_emul(q, k, v, B, Tq, Tk, H, Hkv, hd, causal, scale, mode="mfma", dout=None, rope=None, storage=BF16):
    """The arithmetic the kernels' head comments state, in torch fp32 on the host.  Derived from those comments, not fitted to any output.

    mode "mfma"  (attn_fwd_mfma): fp32 scores from bf16 operands; 64-key tiles with an online softmax -- running max m of the scaled scores,
                 P = exp2(s * scale*log2e - m) in fp32, the ROW SUM is formed from the unrounded P (VALU adds), P is rounded to bf16 as the
                 operand of O += P V, the accumulator is rescaled by exp2(m_old - m_new); O / l is rounded to bf16 once.
    mode "short" (attn_fwd_short): all scores of a row at once, exact two-pass softmax; P is rounded to bf16 and BOTH the row sum that normalises
                 O (an MFMA with an all-ones operand) and O are formed from the rounded P; the LSE takes the fp32 sum of the unrounded P.
    mode "ref"   (attention_ref.hip, impl = 1 / fp32 storage / head dims other than 64 and 128): fp32 throughout, nothing but the stored
                 output is rounded (`storage`).
    lse = (m + log2 l) ln 2 in fp32 ("ref": m + log l).
    Backward (needs dout; Tq == Tk): delta = rowsum(dO * O) from the STORED (rounded) O; P = exp2(s * scale*log2e - lse * log2e);
    dS = P (dP - delta) scale.  "mfma": the dQ kernel rounds dS to bf16 (operand of dQ += dS K); the dK/dV kernel rounds P (operand of
    dV += P^T dO) and dS (operand of dK += dS^T Q); fp32 accumulation over the query tiles AND the query heads of a group; the inverse rotary
    (rope = (cos, sin) fp32) is applied to the fp32 accumulators of dq and dk; one bf16 rounding of each result.  "ref": nothing rounded but
    the stored results.  -> dict(o, lse[, dq, dk, dv]) as fp32 tensors holding the stored values."""
    hm = head_map(H, Hkv)
    q4, k4, v4 = _heads(q, B, Tq, H, hd, F32), _heads(k, B, Tk, Hkv, hd, F32)[:, hm], _heads(v, B, Tk, Hkv, hd, F32)[:, hm]
    vis = visible(Tq, Tk, causal)
    st = (lambda x: x.to(storage).to(F32))
    sl = float(torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E_F32, dtype=F32))
    raw = torch.einsum("bhid,bhjd->bhij", q4, k4).masked_fill(~vis, float("-inf"))
    if mode == "mfma":
        m_run = torch.full(raw.shape[:-1], float("-inf"), dtype=F32)
        l = torch.zeros_like(m_run)
        acc = torch.zeros_like(q4)
        for kb in range(0, Tk, 64):
            t = raw[..., kb:kb + 64]
            m_new = torch.maximum(m_run, t.max(-1).values * sl)
            m_use = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            alpha = torch.exp2(m_run - m_use)
            p = torch.exp2(t * sl - m_use[..., None])
            l = l * alpha + p.sum(-1)
            acc = acc * alpha[..., None] + torch.einsum("bhij,bhjd->bhid", _bf(p), v4[:, :, kb:kb + 64])
            m_run = m_new
        o4 = _bf(acc * (1.0 / l)[..., None])
        lse = (m_run + torch.log2(l)) * LN2_F32
    elif mode == "short":
        m = raw.max(-1).values * sl
        p32 = torch.exp2(raw * sl - m[..., None])
        p = _bf(p32)
        l = p.sum(-1)
        o4 = _bf(torch.einsum("bhij,bhjd->bhid", p, v4) * (1.0 / l)[..., None])
        lse = (m + torch.log2(p32.sum(-1))) * LN2_F32
    elif mode == "ref":
        s = raw * scale
        m = s.max(-1).values
        p = torch.exp(s - m[..., None])
        l = p.sum(-1)
        o4 = st(torch.einsum("bhij,bhjd->bhid", p, v4) * (1.0 / l)[..., None])
        lse = m + torch.log(l)
    else:
        raise KeyError(mode)
    out = {"o": _rows(o4), "lse": lse}
    if dout is None:
        return out
    assert Tq == Tk
    do4 = _heads(dout, B, Tq, H, hd, F32)
    delta = (do4 * o4).sum(-1, keepdim=True)
    dp = torch.einsum("bhid,bhjd->bhij", do4, v4)
    if mode == "ref":
        p = torch.exp(raw * scale - lse[..., None])
        rnd = (lambda x: x)
    else:
        p = torch.exp2(raw * sl - (lse * LOG2E_F32)[..., None])
        rnd = _bf
    p = torch.where(vis, p, torch.zeros_like(p))
    ds = p * (dp - delta) * scale
    dq4 = torch.einsum("bhij,bhjd->bhid", rnd(ds), k4)
    dk4 = _group_sum(torch.einsum("bhij,bhid->bhjd", rnd(ds), q4), Hkv)
    dv4 = _group_sum(torch.einsum("bhij,bhid->bhjd", rnd(p), do4), Hkv)
    if rope is not None:
        dq4, dk4 = unrope(dq4, rope), unrope(dk4, rope)
    out.update(dq=_rows(st(dq4)), dk=_rows(st(dk4)), dv=_rows(st(dv4)))
    return out


# ---------------------------------------------------------------- input families (deterministic, bf16-exact: every precision sees the same tensors)
FAMILIES = ("randn", "flat", "sharp", "sharp_last", "range", "offset", "count")


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def sharp_targets(Tq, Tk, causal, last=False):
    """The dominant key of every query.  Across queries the targets walk over: the first key, the last visible key, both sides of every 64-key
    tile edge and 16-key block edge, and (causal) the diagonal; clamped to what the query sees.  last=True: every query's maximum is its LAST
    visible key, so the online-softmax rescale fires in the final tile."""
    off = Tk - Tq
    lastvis = torch.arange(Tq) + off if causal else torch.full((Tq,), Tk - 1)
    if last:
        return lastvis
    edges = [0, Tk - 1]
    for e in range(16, Tk, 16):
        edges += [e - 1, e]
    edges = torch.tensor(sorted(set(edges)))
    tgt = edges[torch.arange(Tq) % len(edges)]
    if causal:
        diag = torch.arange(Tq) % 3 == 0                     # every third query: its own diagonal key
        tgt = torch.where(diag, lastvis, tgt)
    return torch.minimum(tgt, lastvis)


def make_inputs(fam, B, Tq, Tk, H, Hkv, hd, causal, seed=0, bwd_count=False):
    """-> q [B*Tq, H*hd], k, v [B*Tk, Hkv*hd], dout [B*Tq, H*hd], bf16 on the CPU.  scale is hd^-0.5 throughout.
    count: K = 0 (every score 0, P exactly uniform over the visible keys), V small integers that differ per kv head and batch item;
    bwd_count=True makes every K row the same NONZERO vector instead (P still uniform; dk is then not identically zero)."""
    g = _gen(1000 * seed + 7 * Tq + 13 * Tk + hd + 3 * H + Hkv)
    q = torch.randn(B, Tq, H, hd, generator=g)
    k = torch.randn(B, Tk, Hkv, hd, generator=g)
    v = torch.randn(B, Tk, Hkv, hd, generator=g)
    dout = torch.randn(B, Tq, H, hd, generator=g)
    if fam == "randn":
        pass
    elif fam == "flat":
        q = q * 0.05
    elif fam in ("sharp", "sharp_last"):
        # q_i = 2 * (unit-ish direction of its target key) * sqrt(hd)-normalised: score of the target ~ 2 |k|^2 / sqrt(hd) ~ 2 sqrt(hd) above the rest
        tgt = sharp_targets(Tq, Tk, causal, fam == "sharp_last")
        kq = k[:, tgt][:, :, head_map(H, Hkv)]                # [B, Tq, H, hd]: the target key of each query, in its own kv head
        q = 2.0 * kq + 0.1 * q
    elif fam == "range":
        # scores spread over about +-60 after scaling: |q.k| hd^-0.5 with q, k ~ N(0, s^2) has std s^2; s^2 = 20 -> 3 sigma = 60
        q, k = q * 20 ** 0.5, k * 20 ** 0.5
    elif fam == "offset":
        v = v + 8.0
    elif fam == "count":
        k = torch.zeros_like(k)
        if bwd_count:
            k = k + torch.randn(1, 1, 1, hd, generator=g).to(BF16).float()
        v = torch.randint(-4, 5, (B, Tk, Hkv, hd), generator=g).float()
        v = v + (torch.arange(Hkv).float()[None, None, :, None] % 3 - 1) + (torch.arange(B).float()[:, None, None, None] % 2)   # head / item show
        v = v.clamp(-4, 4)
    else:
        raise KeyError(fam)
    r = (lambda x, T, h: x.reshape(B * T, h * hd).to(BF16))
    return r(q, Tq, H), r(k, Tk, Hkv), r(v, Tk, Hkv), r(dout, Tq, H)


def visible_counts(Tq, Tk, causal):
    """n_i of the count family: i + 1 + Tk - Tq under the causal mask, Tk otherwise."""
    return visible(Tq, Tk, causal).sum(-1)


# ---------------------------------------------------------------- geometry table of tests/test_attention_pin_gpu.py
# form: the kernel av_attention_fwd selects; emul: attn_emul's mode; knob: ATTN_SHORT = 0 forces the general kernel; dt / impl as passed.
Geo = namedtuple("Geo", "form B Tq Tk H Hkv hd causal emul knob dt impl")


def _g(form, T, hd, causal, emul, B=2, H=2, Hkv=None, Tk=None, knob=False, dt="bf16", impl=0):
    return Geo(form, B, T, T if Tk is None else Tk, H, H if Hkv is None else Hkv, hd, causal, emul, knob, dt, impl)


GEOMETRIES = []
GEOMETRIES += [_g("short13x7", T, 64, False, "short") for T in (1, 15, 16, 17, 197, 208)]
GEOMETRIES += [_g("short17x9", T, 64, False, "short") for T in (209, 257, 272)]
GEOMETRIES += [_g("mfma64x4", T, 64, False, "mfma") for T in (273, 330)]
GEOMETRIES += [_g("mfma64x4", T, 64, True, "mfma") for T in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)]
GEOMETRIES += [_g("mfma64x4", T, 64, False, "mfma", knob=True) for T in (129, 197, 224)]       # short lengths on the general kernel (the knob)
GEOMETRIES += [_g("tqtk-mfma64x4", 150, 64, False, "mfma", Tk=200)]                              # and without it where Tk != Tq
GEOMETRIES += [_g("mfma128x4", T, 128, c, "mfma") for c in (True, False) for T in (1, 33, 64, 65, 129, 257)]
GEOMETRIES += [_g("gqa-mfma128x4", 70, 128, True, "mfma", B=2, H=H, Hkv=Hkv) for H, Hkv in ((4, 2), (4, 1), (8, 1))]
GEOMETRIES += [_g("gqa-short13x7", 50, 64, False, "short", B=3, H=4, Hkv=2), _g("gqa-mfma64x4", 130, 64, True, "mfma", B=2, H=8, Hkv=2)]
GEOMETRIES += [_g("tqtk-mfma%dx4" % hd, Tq, hd, True, "mfma", Tk=Tk) for hd in (64, 128) for Tq, Tk in ((1, 65), (32, 96), (33, 130), (70, 257))]
GEOMETRIES += [_g("tqtk-mfma%dx4" % hd, 50, hd, False, "mfma", Tk=197) for hd in (64, 128)]
GEOMETRIES += [_g("ref", 40, hd, c, "ref", dt=dt) for dt in ("f32", "bf16") for hd in (32, 96, 512) for c in (True, False)]
GEOMETRIES += [_g("ref-impl1", 70, hd, True, "ref", dt=dt, impl=1) for dt in ("f32", "bf16") for hd in (64, 128)]
GEOMETRIES += [_g("ref-f32", T, hd, c, "ref", dt="f32") for T, hd, c in ((197, 64, False), (65, 128, True))]


def kernel_of(g):
    """The name (avllm.lib.ATTN_FORMS) of the kernel g.form stands for: the form without its gqa- / tqtk- / rope-bwd- / -impl1 / -f32 decorations."""
    return next(k for k in ("short13x7", "short17x9", "mfma64x4", "mfma128x4", "ref") if k in g.form.split("-"))


def geo_id(g):
    return (f"{g.form}-{g.dt}-hd{g.hd}-{'causal' if g.causal else 'full'}-Tq{g.Tq}-Tk{g.Tk}-B{g.B}-H{g.H}-Hkv{g.Hkv}"
            + ("-impl1" if g.impl else "") + ("-short_off" if g.knob else ""))


def head_cols(g, name):
    """The column slice of every head of a backward tensor: dq has g.H heads, dk and dv g.Hkv."""
    return [slice(h * g.hd, (h + 1) * g.hd) for h in range(g.H if name == "dq" else g.Hkv)]


def bwd_ratio(c, g, name, x):
    """max |x - ref| / bar of backward tensor `name` (dq, dk, dv): over the whole tensor against bar_<name> and over every head slice against that
    head's own hbar_<name>; inf if x is not finite."""
    err = (x.detach().double().cpu() - getattr(c, name + "64")).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    r = float(err.max()) / getattr(c, "bar_" + name)
    return max([r] + [float(err[:, s].max()) / hb for s, hb in zip(head_cols(g, name), getattr(c, "hbar_" + name))])


def has_bwd(g):
    """The backward takes one T, and the scalar backward stops at head_dim 128."""
    return g.Tq == g.Tk and not (g.emul == "ref" and g.hd > 128)


# ---------------------------------------------------------------- one case = inputs + float64 reference + bars (shared by the CPU and the GPU file)
class Case:
    pass


_CASES = {}


def case(g, fam, rope=None, rope_key=None):
    """Inputs, float64 reference, host emulation and the bars of tests/bars.py for geometry g and family fam; computed once and never modified.
    Forward: o64, lse64, bar_o (elementwise), bar_lse (elementwise or a number).  Backward (has_bwd(g)): the inputs bq / bk / bv / bdout (the count
    family swaps K = 0 for K = one nonzero row), ref dq64 / dk64 / dv64, per-tensor bars bar_d*, the same rule per head slice hbar_d* (a list),
    rel_l2_d*, and for the count family the elementwise ebar_d*.  emul: attn_emul's dict for the forward inputs, emul_b for the backward's."""
    import bars as Bar
    key = (g, fam, rope_key)
    if key in _CASES:
        return _CASES[key]
    c = Case()
    B, Tq, Tk, H, Hkv, hd, causal = g.B, g.Tq, g.Tk, g.H, g.Hkv, g.hd, g.causal
    c.scale = hd ** -0.5
    c.storage = BF16 if g.dt == "bf16" else F32
    rounded = g.dt == "bf16"
    c.q, c.k, c.v, c.dout = make_inputs(fam, B, Tq, Tk, H, Hkv, hd, causal)
    args = (B, Tq, Tk, H, Hkv, hd, causal, c.scale)
    c.o64, c.lse64, w = attn_fwd64(c.q, c.k, c.v, *args)
    o32, lse32, _ = attn_fwd64(c.q, c.k, c.v, *args, dtype=F32)
    c.emul = attn_emul(c.q, c.k, c.v, *args, mode=g.emul, storage=c.storage)
    if fam == "count":
        n = visible_counts(Tq, Tk, causal)
        c.bar_o = Bar.attn_count_out_bar(c.o64, rounded)
        c.bar_lse = Bar.attn_count_lse_bar(n)[None, None, :].expand(B, H, Tq)
        c.n = n
    else:
        fb = Bar.fp32_bar(c.o64, o32)
        term = None
        if rounded and g.emul != "ref":
            v4 = _heads(c.v, B, Tk, Hkv, hd, F64)[:, head_map(H, Hkv)]
            o4 = _heads(c.o64, B, Tq, H, hd, F64)
            if g.emul == "short":
                term = torch.stack([(w[..., None] * (v4[:, :, None, :, d0:d0 + 16] - o4[:, :, :, None, d0:d0 + 16]).abs()).sum(3)
                                    for d0 in range(0, hd, 16)], -1).permute(0, 1, 2, 4, 3).reshape(B, H, Tq, hd)
            else:
                term = torch.einsum("bhij,bhjd->bhid", w, v4.abs())
            term = _rows(term)
        c.bar_o = Bar.attn_out_bar(c.o64, term, fb, rounded)
        c.bar_lse = Bar.attn_lse_bar(c.lse64, lse32, Tk)
    if has_bwd(g):
        T = Tq
        if fam == "count":
            c.bq, c.bk, c.bv, c.bdout = make_inputs(fam, B, T, T, H, Hkv, hd, causal, bwd_count=True)
        else:
            c.bq, c.bk, c.bv, c.bdout = c.q, c.k, c.v, c.dout
        bargs = (B, T, H, Hkv, hd, causal, c.scale)
        c.dq64, c.dk64, c.dv64 = attn_bwd64(c.bq, c.bk, c.bv, c.bdout, *bargs, rope=rope)
        c.emul_b = attn_emul(c.bq, c.bk, c.bv, B, T, T, H, Hkv, hd, causal, c.scale, mode=g.emul, dout=c.bdout, rope=rope, storage=c.storage)
        if rounded:
            yard = (c.emul_b["dq"], c.emul_b["dk"], c.emul_b["dv"])
            amp = delta_amplification(c.bq, c.bk, c.bv, c.bdout, *bargs)
            c.rel_l2_dq = c.rel_l2_dk = Bar.attn_bwd_rel_l2_bar(amp)
            c.rel_l2_dv = Bar.attn_bwd_rel_l2_bar(0.0)
            if fam in ("sharp", "sharp_last"):
                # a one-hot softmax makes dS = P (dP - delta) a cancellation: dq and dk are SMALLER than the rounding of delta (relative error of order
                # 1 is the arithmetic's own, in the emulation too), so only the absolute bars, per tensor and per head, say anything there; dv is unaffected
                c.rel_l2_dq = c.rel_l2_dk = None
            if fam == "count":
                c.rel_l2_dq = None                           # dq is identically zero in this family
        else:
            yard = attn_bwd64(c.bq, c.bk, c.bv, c.bdout, *bargs, rope=rope, dtype=F32)
            c.rel_l2_dq = c.rel_l2_dk = c.rel_l2_dv = None
        # per tensor and per head slice of it (dq: query heads; dk, dv: kv heads, so a group sum that lands on the wrong head shows against that
        # head's own bar): Bar.attn_bwd_tensor_bar = the yardstick rule + the derived fp32 bound underneath; dq and dk are rotated when rope is given
        under = Bar.attn_bwd_elem_bars(c.bq, c.bk, c.bv, c.bdout, *bargs, rounded=False, p_rounded=False)
        for name, r64, y, u_ in zip(("dq", "dk", "dv"), (c.dq64, c.dk64, c.dv64), yard, under):
            rot = rope is not None and name != "dv"
            setattr(c, "bar_" + name, Bar.attn_bwd_tensor_bar(r64, y, u_, rounded, rot))
            setattr(c, "hbar_" + name, [Bar.attn_bwd_tensor_bar(r64[:, s], y[:, s], u_[:, s], rounded, rot) for s in head_cols(g, name)])
        if fam == "count":
            c.ebar_dq, c.ebar_dk, c.ebar_dv = Bar.attn_bwd_elem_bars(c.bq, c.bk, c.bv, c.bdout, *bargs, rounded=rounded,
                                                                    p_rounded=rounded and g.emul != "ref")
    _CASES[key] = c
    return c
