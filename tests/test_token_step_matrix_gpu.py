"""The token step of LlamaEngine (csrc/engine.hip llama_decode_layer_fused) on every case of tests/token_step_cases.py: weight stream x cache
form x head norms x biases x adapters x head geometry x RoPE rule x host / device position x copy cache / shared prefix (one launch, sliced)
x row count, against the float64 reference of tests/refs64_kv8.py.  tests/test_token_step_cases_cpu.py shows on the host that the case list
holds every pair of levels, that the reference is transformers' arithmetic, that a correct bf16 step has half the bar to itself in every case
and that a step with one feature wrong misses the bar by far.

Per case: the prefill logits against the reference's prefill; then the reference starts from the rows the engine's prefill STORED (read back,
dequantised for an fp8 image), runs the five teacher-forced steps in the case's cache form on the weights the steps multiply, with the
parents applied, and every step's logits are held to BF16_LOGITS_REL_L2 and BF16_LOGIT_MAX_ABS.  Layer 0's k and v of a new token depend on
the token and its position only, so a twin engine with a bf16 copy cache gives the rows the steps must have written:

  * a bf16 cache holds the twin's rows bit for bit, an fp8 image holds oracle.mxfp8.quantize of them, codes and exponents both -- v always,
    k wherever the two engines round at the same places (bf16 cache; fp8 cache with head norms, whose launch leaves the rotated bf16 k);
  * the k image of an fp8 cache WITHOUT head norms cannot be stated bit for bit from the twin: kv8_rope_append_kernel rotates the bf16 raw k
    in fp32 and quantises without a bf16 rounding in between (csrc/kv_fp8.hip), the twin's epilogue rotates the fp32 raw k and rounds once.
    With u = 2^-8 (a bf16 rounding) and rho the norm of a rotary pair, the rotation of rounded inputs is within u rho of the exact one
    (Cauchy-Schwarz over |c|, |s|) and the twin's rounding within u rho too: the quantiser's input y is within delta = 2 u rho (1 + 2^-6)
    of the twin's value t.  So the block exponent is the rule's for some maximum in [max(|t| - delta), max(|t| + delta)], and under it
    every element is within delta + half an e4m3 step (2^-4 relative, 2^-10 2^e in the subnormal range, 2^-3 where the clamp at 448 acts)
    of t.  The share of codes that equal the plain rule's is printed (measured on MI355X in the four such cases: every exponent, and
    0.9516 .. 0.9672 of the codes).

After the loop the positions past the last written one hold their fill (NaN, or 0xA5 in an image) and a shared prefix cache is what the
prefill left."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import refs64_kv8 as R  # noqa: E402
import token_step_cases as TC  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402
from bars import BF16_U  # noqa: E402
from oracle import mxfp8  # noqa: E402

BF = torch.bfloat16
S, NEW = TC.S, TC.NEW


def fill(*caches):
    for t in caches:
        t.fill_(0xA5) if t.dtype == torch.uint8 else t.fill_(float("nan"))


def holds_fill(t):
    """Every element of a slice of a cache (or of a plane of an image) is the fill value."""
    nan = int(torch.tensor([float("nan")], dtype=BF).view(torch.int16)[0])
    return bool((t == 0xA5).all()) if t.dtype == torch.uint8 else bool((t.view(torch.int16) == nan).all())


def planes(c):
    return ops.kv8_unpack(c) if c.dtype == torch.uint8 else (c,)


def stored(cache, lo, hi):
    """Positions [lo, hi) of a cache [layers, rows, T, dkv] as the values a reader gets, float64 on the host."""
    if cache.dtype != torch.uint8:
        return cache[:, :, lo:hi].double().cpu()
    q, e = ops.kv8_unpack(cache)
    return R.mx_dequantize64(q[:, :, lo:hi].cpu(), e[:, :, lo:hi].cpu().to(torch.int32) - 127)


def as_past(c, k, v):
    """Stored rows [layers, rows, T, dkv] -> the reference's past: per layer (k, v) [rows, Hkv, T, hd]."""
    hd = c.hidden // c.heads
    sp = lambda t: t.view(t.shape[0], t.shape[1], c.kv_heads, hd).transpose(1, 2)      # noqa: E731
    return [(sp(k[i]), sp(v[i])) for i in range(c.layers)]


def k_image_follows_the_twin(c, q, e, t):
    """The derived check of the module docstring: q, e = codes and unbiased exponents [R, NEW, dkv], [R, NEW, dkv / 32] of an fp8 k image written
    without head norms, t = the twin's bf16 rows.  Returns the share of codes equal to the plain rule's."""
    hd = c.hidden // c.heads
    t = t.double()
    th = t.view(*t.shape[:-1], c.kv_heads, 2, hd // 2)
    rho = (th[..., 0, :] ** 2 + th[..., 1, :] ** 2).sqrt()
    delta = (2.0 * BF16_U * (1.0 + 2.0 ** -6) * torch.stack([rho, rho], -2)).reshape(t.shape)
    blk = lambda x: x.reshape(*x.shape[:-1], x.shape[-1] // 32, 32)      # noqa: E731
    lo, hi = blk((t.abs() - delta).clamp_min(0.0)).amax(-1), blk(t.abs() + delta).amax(-1)
    assert bool((lo > 0).all()), "a block of k that may be all zero: the case's draw is not what this check assumes"
    e_lo, e_hi = torch.frexp(lo)[1] - 1 - 8, torch.frexp(hi)[1] - 1 - 8
    assert bool(((e >= e_lo) & (e <= e_hi)).all()), "a block exponent no maximum within delta of the twin's row gives"
    got = R.mx_dequantize64(q, e)
    scale = torch.ldexp(torch.ones((), dtype=torch.float64), e).unsqueeze(-1).expand(*e.shape, 32).reshape(t.shape)
    y = t.abs() + delta
    half = torch.where(y > 448.0 * scale, 2.0 ** -3 * y, torch.maximum(2.0 ** -4 * y, 2.0 ** -10 * scale))
    worst = float(((got - t).abs() / (delta + half)).max())
    assert worst <= 1.0, f"a k image element {worst:.2f} x further from the twin's row than the roundings and the e4m3 step allow"
    wq, we = mxfp8.quantize(t.float())
    return float((wq == q).double().mean()), float((we == e).double().mean())


@pytest.mark.parametrize("c", TC.CASES, ids=lambda c: c.id)
def test_token_step_matrix(dev, c):
    from avllm.arch import LoraCfg
    from avllm.engine import LlamaEngine
    sd, lora = TC.weights(c)
    cfg = TC.llama_cfg(c)
    lc = LoraCfg(c.lora, 2.0 * c.lora) if c.lora else None
    eng = LlamaEngine(sd, cfg, lc, lora, dtype=BF, device=dev, training=False, **TC.engine_kwargs(c))
    Rr, fp8c = c.R, c.cache == "fp8"
    # ---- predicates (decode_shares_prefix is the fused step's capability: true in copy cases too)
    assert eng.decode_is_fused(Rr) and eng.decode_shares_prefix(Rr)
    assert eng.decode_streams_fp8(Rr) == (c.weights == "fp8") and eng.decode_streams_fp4(Rr) == (c.weights == "fp4")
    assert eng.decode_caches_fp8(Rr) == fp8c
    assert bool(all(ly.q_norm_w for ly in eng.layers)) == bool(c.norms) and bool(all(ly.bqkv for ly in eng.layers)) == (c.bias != "none")
    assert bool(all(ly.bo for ly in eng.layers)) == (c.bias == "qkvo")

    x, tokens = TC.inputs(c)
    xg, ids = x.to(dev, BF), tokens.to(dev)
    N = NEW + TC.PAD
    if c.shared:
        kp, vp = eng.alloc_cache(c.items, S, rows=Rr)
        ks, vs = eng.alloc_suffix_cache(Rr, N)
        fill(kp, vp, ks, vs)
        kw, vw, w0 = ks, vs, 0                                   # where the steps write: cache pair, first position
    else:
        kp, vp = eng.alloc_cache(Rr, S + N)
        fill(kp, vp)
        kw, vw, w0 = kp, vp, S
    assert kp.dtype == kw.dtype == (torch.uint8 if fp8c else BF)
    last, _ = eng.prefill(xg, kp, vp)
    kp0, vp0 = kp.clone(), vp.clone()

    # ---- prefill logits: the reference on the original weights, attention over its own rows
    want0, _ = TC.ref_prefill(c, sd, lora, x)
    worst = max(TC.ratios(last.cpu(), want0))
    print(f"RATIO {c.id} prefill {worst:.3f}")
    assert worst < 1.0

    # ---- the steps
    gather = ops.kv8_gather_rows if fp8c else ops.kv_gather_rows
    pd = torch.zeros(1, device=dev, dtype=torch.int32) if c.pos == "dev" else None
    got = []
    for t in range(NEW):
        tok = ids[:, t].contiguous()
        if pd is not None:
            pd.fill_(t)
        if c.shared:
            p = TC.parents(c, t)
            if p is not None:
                gather(ks, vs, ks, vs, p.to(dev, torch.int32).contiguous(), 0, t)
            with L.knob("SHARED_SPLIT", c.split):
                out = eng.decode_step_shared(tok, 0 if pd is not None else t, kp, vp, ks, vs, c.group, pos_dev=pd)
        else:
            out = eng.decode_step(tok, S if pd is not None else S + t, kp, vp, pos_dev=pd)
        got.append(out.clone())
    got = torch.stack(got, 1).cpu()

    # ---- the reference from the rows the prefill stored
    past = TC.rows_of(c, as_past(c, stored(kp0, 0, S), stored(vp0, 0, S)))
    want = TC.ref_steps(c, TC.step_weights(c, sd), lora, past, tokens)
    ratio = [TC.ratios(got[:, t], want[:, t]) for t in range(NEW)]
    for t in range(NEW):
        print(f"RATIO {c.id} step {t} {max(ratio[t]):.3f} (relative L2 {ratio[t][0]:.3f}, max abs {ratio[t][1]:.3f} of their bars)")
    assert max(max(r) for r in ratio) < 1.0, ratio

    # ---- layer 0's new rows against a twin with a bf16 copy cache
    twin = eng if not fp8c else LlamaEngine(sd, cfg, lc, lora, dtype=BF, device=dev, training=False, **dict(TC.engine_kwargs(c), kv_fp8=False))
    tk, tv = twin.alloc_cache(Rr, S + NEW)
    twin.prefill(xg.repeat_interleave(c.group, 0).contiguous(), tk, tv)
    for t in range(NEW):
        twin.decode_step(ids[:, t].contiguous(), S + t, tk, tv)
    src = TC.lineage(c)
    col = torch.arange(NEW)[None, :].expand(Rr, NEW)
    for name, cache, tw in (("k", kw, tk), ("v", vw, tv)):
        rows = tw[0, :, S:S + NEW].cpu()[src, col]               # [R, NEW, dkv]: position j of row r is what row src[r, j] wrote at step j
        assert cache.dtype == (torch.uint8 if fp8c else BF) and bool(torch.isfinite(rows.float()).all())
        if not fp8c:
            mine = cache[0, :, w0:w0 + NEW].cpu()
            assert torch.equal(mine.view(torch.int16), rows.view(torch.int16)), f"layer-0 {name} rows are not the twin's"
            continue
        q, e = (pl[0, :, w0:w0 + NEW].cpu() for pl in ops.kv8_unpack(cache))
        e = e.to(torch.int32) - 127
        if name == "k" and not c.norms:
            same = k_image_follows_the_twin(c, q, e, rows)
            print(f"{c.id}: k image without head norms: {same[0]:.4f} of the codes and {same[1]:.4f} of the exponents are the plain rule's of the twin's rows")
            continue
        wq, we = mxfp8.quantize(rows.float())
        assert torch.equal(q, wq) and torch.equal(e, we), f"layer-0 {name} image is not the MX rule of the twin's rows"

    # ---- nothing else was written
    for cache in (kw, vw):
        for pl in planes(cache):
            assert holds_fill(pl[:, :, w0 + NEW:]), "a position past the last written one lost its fill"
    if c.shared:
        assert torch.equal(kp.view(torch.uint8), kp0.view(torch.uint8)) and torch.equal(vp.view(torch.uint8), vp0.view(torch.uint8)), "the steps wrote into the prefix cache"
        for cache in (kp0, vp0):
            assert bool(torch.isfinite(stored(cache, 0, S)).all())
