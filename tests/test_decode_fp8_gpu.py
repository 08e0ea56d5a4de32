"""Weight-only fp8 token step: avllm_mx_quantize layout 2 (row-major E8M0 exponents), the fp8 weight form of avllm_dec_proj and the engine's
decode_fp8 mode.  Numerics definition: the fp8 form computes what the bf16 form computes on W~ = dequantize(codes, exponents), which is an
ordinary (exactly representable) bf16 weight set; only the fp32 summation order inside a pair of K-steps differs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from avllm import ops  # noqa: E402
from bars import rel_l2  # noqa: E402
from oracle import mxfp8  # noqa: E402
from test_ops_gpu import rnd  # noqa: E402

BF = torch.bfloat16


def rms(x, w, eps):
    x = x.float()
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w.float()


def fp8_weights(W):
    """(codes, exponents) of the kernel's quantiser (layout 2) and W~ as a bf16 tensor (exact)."""
    q, e = ops.mx_quantize(W, 2)
    wt = mxfp8.dequantize(q.cpu(), e.cpu().to(torch.int32) - 127)
    wt16 = wt.to(BF)
    assert torch.equal(wt16.float(), wt)                  # W~ is a bf16 weight set
    return q, e, wt16.to(W.device)


def within_one_ulp(a, b):
    """bf16 tensors a, b differ by at most one unit in the last place of the larger magnitude."""
    a, b = a.float(), b.float()
    mag = torch.maximum(a.abs(), b.abs()).clamp_min(2.0 ** -126)
    ulp = torch.ldexp(torch.ones_like(mag), torch.floor(torch.log2(mag)).to(torch.int32) - 7)
    return bool(((a - b).abs() <= ulp).all())


# ------------------------------------------------------------------------------------------------ 1. exponents
@pytest.mark.parametrize("R,K", [(16, 128), (16, 11008), (4608, 4096), (4608, 11008), (32000, 128), (32000, 4096)])
def test_layout2_exponents_and_codes_match_the_oracle(dev, R, K):
    W = rnd(R, K, dtype=BF, seed=7, scale=K ** -0.5)
    W[:3, :32] = 0                                        # an all-zero block: exponent -127 (biased 0)
    q, e = ops.mx_quantize(W, 2)
    assert e.shape == (R, K // 32) and e.dtype == torch.uint8
    assert torch.equal(e.cpu().to(torch.int32), mxfp8.block_exponents(W.cpu().float()) + 127)
    codes, _ = mxfp8.quantize(W.cpu().float())
    assert torch.equal(q.cpu(), codes)
    q1, _ = ops.mx_quantize(W, 1)                         # the codes are the GEMM images' codes
    assert torch.equal(q1, q)


# ------------------------------------------------------------------------------------------------ 2. dec_proj fp8 vs torch on W~
# K: groups per wave 0 / 1 (128), 2 / 1 (1152), 3 / 2 (2944), 4 (4096), 5 (5120), 11 / 10 (11008): with the ring of 2 groups these reach every
# length of the straight-line tail, 1 .. 3, with and without a trip of the main loop before it
@pytest.mark.parametrize("K", [128, 1152, 2944, 4096, 5120, 11008])
@pytest.mark.parametrize("M", [1, 4, 5, 8, 16])
def test_dec_proj_fp8_plain_norm_residual(dev, M, K):
    N = 528
    A, W = rnd(M, K, dtype=BF, seed=1), rnd(N, K, dtype=BF, seed=2, scale=K ** -0.5)
    R, g = rnd(M, N, dtype=BF, seed=3), (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=4)).to(BF)
    q, e, wt = fp8_weights(W)
    ref = A.float() @ wt.float().t()
    assert rel_l2(ops.dec_proj(A, None, W8=q, E8=e, out_f32=True), ref) < 2e-3
    out = R.clone()
    ops.dec_proj(A, None, W8=q, E8=e, R=out, out=out)
    assert rel_l2(out, ref + R.float()) < 6e-3
    refn = rms(A, g, 1e-5) @ wt.float().t()
    assert rel_l2(ops.dec_proj(A, None, W8=q, E8=e, norm_w=g, eps=1e-5, out_f32=True), refn) < 6e-3
    rows = rnd(4 * M, K, dtype=BF, seed=5)
    assert rel_l2(ops.dec_proj(rows[3::4], None, W8=q, E8=e, out_f32=True), rows[3::4].float() @ wt.float().t()) < 2e-3


@pytest.mark.parametrize("M,al", [(1, "2"), (1, "4"), (3, "4"), (4, "2"), (5, "4"), (8, "4")])
def test_dec_proj_fp8_activation_load_forms(dev, M, al):
    """The forced wider activation-load forms (AVLLM_DEC_AL) give bit-identical sums: the same elements meet in the same order."""
    K = 2944
    A, W = rnd(M, K, dtype=BF, seed=1), rnd(528, K, dtype=BF, seed=2, scale=K ** -0.5)
    g = (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=4)).to(BF)
    q, e, wt = fp8_weights(W)
    want = ops.dec_proj(A, None, W8=q, E8=e, out_f32=True), ops.dec_proj(A, None, W8=q, E8=e, norm_w=g, eps=1e-5, out_f32=True)
    with ops.L.knob("DEC_AL", int(al)):
        got = ops.dec_proj(A, None, W8=q, E8=e, out_f32=True), ops.dec_proj(A, None, W8=q, E8=e, norm_w=g, eps=1e-5, out_f32=True)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    assert rel_l2(want[0], A.float() @ wt.float().t()) < 2e-3
    assert rel_l2(want[1], rms(A, g, 1e-5) @ wt.float().t()) < 6e-3


@pytest.mark.parametrize("M,K,F", [(1, 256, 64), (8, 4096, 11008), (16, 1152, 520), (5, 11008, 128)])
def test_dec_proj_fp8_swiglu(dev, M, K, F):
    A, W = rnd(M, K, dtype=BF, seed=11), rnd(2 * F, K, dtype=BF, seed=12, scale=K ** -0.5)
    g = (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=13)).to(BF)
    q, e, wt = fp8_weights(W)
    xn = rms(A, g, 1e-6)
    gate, up = xn @ wt[:F].float().t(), xn @ wt[F:].float().t()
    out = ops.dec_proj(A, None, mode=1, norm_w=g, eps=1e-6, W8=q, E8=e)
    assert out.shape == (M, F) and rel_l2(out, torch.nn.functional.silu(gate) * up) < 8e-3


def _rope(dev, hd, pos):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, device=dev).float() / hd))
    ang = pos * inv
    return ang, torch.stack([ang.cos(), ang.sin()], -1).contiguous()


def _rot(t, ang, M, nh, hd):
    t = t.view(M, nh, hd)
    a, b = t[..., : hd // 2], t[..., hd // 2:]
    return torch.cat([a * ang.cos() - b * ang.sin(), b * ang.cos() + a * ang.sin()], -1).reshape(M, nh * hd)


@pytest.mark.parametrize("M,heads,kvh,hd,K", [(1, 4, 4, 128, 128), (8, 4, 2, 64, 256), (16, 8, 2, 128, 1024), (4, 32, 8, 128, 4096)])
def test_dec_proj_fp8_qkv_rope_cache(dev, M, heads, kvh, hd, K):
    dq, dkv, Tmax, pos = heads * hd, kvh * hd, 9, 5
    A, W = rnd(M, K, dtype=BF, seed=21), rnd(dq + 2 * dkv, K, dtype=BF, seed=22, scale=K ** -0.5)
    g = (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=23)).to(BF)
    q8, e8, wt = fp8_weights(W)
    ang, rope = _rope(dev, hd, pos)
    y = rms(A, g, 1e-5) @ wt.float().t()
    for use_dev in (False, True):
        kc = torch.full((M, Tmax, dkv), 7.0, device=dev, dtype=BF)
        vc = torch.full((M, Tmax, dkv), -7.0, device=dev, dtype=BF)
        pd = torch.tensor([3], device=dev, dtype=torch.int32) if use_dev else None
        q = ops.dec_proj(A, None, mode=2, norm_w=g, eps=1e-5, rope=rope, kc=kc, vc=vc, pos=pos - (3 if use_dev else 0), pos_dev=pd, dq=dq, dkv=dkv,
                         hd=hd, W8=q8, E8=e8)
        assert rel_l2(q, _rot(y[:, :dq], ang, M, heads, hd)) < 8e-3
        assert rel_l2(kc[:, pos], _rot(y[:, dq:dq + dkv], ang, M, kvh, hd)) < 8e-3
        assert rel_l2(vc[:, pos], y[:, dq + dkv:]) < 8e-3
        keep = [t for t in range(Tmax) if t != pos]
        assert (kc[:, keep] == 7.0).all() and (vc[:, keep] == -7.0).all()


@pytest.mark.parametrize("M,r", [(1, 16), (5, 8), (16, 4)])
def test_dec_proj_fp8_adapter_side_term(dev, M, r):
    """peft lora.Linear on the fp8 token step: the base product streams codes, the rank-side products and B images stay bf16."""
    K, scale = 1152, 2.0
    g = (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=43)).to(BF)
    A = rnd(M, K, dtype=BF, seed=41)
    N = 528
    W = rnd(N, K, dtype=BF, seed=42, scale=K ** -0.5)
    q8, e8, wt = fp8_weights(W)
    Ap = torch.zeros(64, K, device=dev, dtype=BF); Ap[:r] = rnd(r, K, dtype=BF, seed=44, scale=K ** -0.5)
    Bp = torch.zeros(N, 64, device=dev, dtype=BF); Bp[:, :r] = rnd(N, r, dtype=BF, seed=45, scale=0.3)
    R = rnd(M, N, dtype=BF, seed=46)
    t = torch.zeros(M, 256, device=dev, dtype=torch.float32)
    ops.dec_proj(A, Ap[:16], out=t[:, 192:208], out_f32=True)
    ref_t = A.float() @ Ap[:16].float().t()
    out = ops.dec_proj(A, None, W8=q8, E8=e8, R=R, lora_t=t[:, 192:], lora_b=[Bp], lora_r=r, lora_scale=scale, out_f32=True)
    ref = A.float() @ wt.float().t() + R.float() + scale * (ref_t[:, :r] @ Bp[:, :r].float().t())
    assert rel_l2(out, ref) < 3e-3
    # q|k|v with norm + RoPE + cache and the three adapters
    heads, kvh, hd, Tmax, pos = 4, 2, 64, 6, 3
    dq, dkv = heads * hd, kvh * hd
    Wq = rnd(dq + 2 * dkv, K, dtype=BF, seed=47, scale=K ** -0.5)
    q8, e8, wqt = fp8_weights(Wq)
    A3 = torch.zeros(192, K, device=dev, dtype=BF)
    Bs = []
    for j, rows in enumerate((dq, dkv, dkv)):
        A3[64 * j:64 * j + r] = rnd(r, K, dtype=BF, seed=50 + j, scale=K ** -0.5)
        b = torch.zeros(rows, 64, device=dev, dtype=BF); b[:, :r] = rnd(rows, r, dtype=BF, seed=60 + j, scale=0.3)
        Bs.append(b)
    ops.dec_proj(A, A3, norm_w=g, eps=1e-5, out=t[:, :192], out_f32=True)
    xn = rms(A, g, 1e-5)
    y = xn @ wqt.float().t()
    off = 0
    for j, rows in enumerate((dq, dkv, dkv)):
        y[:, off:off + rows] += scale * ((xn @ A3[64 * j:64 * j + r].float().t()) @ Bs[j][:, :r].float().t())
        off += rows
    ang, rope = _rope(dev, hd, pos)
    kc = torch.zeros(M, Tmax, dkv, device=dev, dtype=BF); vc = torch.zeros_like(kc)
    q = ops.dec_proj(A, None, mode=2, norm_w=g, eps=1e-5, rope=rope, kc=kc, vc=vc, pos=pos, dq=dq, dkv=dkv, hd=hd,
                     lora_t=t, lora_b=Bs, lora_r=r, lora_scale=scale, W8=q8, E8=e8)
    assert rel_l2(q, _rot(y[:, :dq], ang, M, heads, hd)) < 8e-3
    assert rel_l2(kc[:, pos], _rot(y[:, dq:dq + dkv], ang, M, kvh, hd)) < 8e-3
    assert rel_l2(vc[:, pos], y[:, dq + dkv:]) < 8e-3


# ------------------------------------------------------------------------------------------------ 3. same order as bf16 on W~
@pytest.mark.parametrize("K", [128, 4096, 11008])
@pytest.mark.parametrize("M", [1, 5, 8, 16])
def test_dec_proj_fp8_matches_bf16_form_on_dequantised_weights(dev, M, K):
    """fp8 form vs the bf16 form over W~: the products are identical, only the fp32 grouping inside pairs of K-steps differs."""
    N = 528
    A, W = rnd(M, K, dtype=BF, seed=31), rnd(N, K, dtype=BF, seed=32, scale=K ** -0.5)
    R, g = rnd(M, N, dtype=BF, seed=33), (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=34)).to(BF)
    q, e, wt = fp8_weights(W)
    a = ops.dec_proj(A, None, W8=q, E8=e, norm_w=g, eps=1e-5, out_f32=True)
    b = ops.dec_proj(A, wt, norm_w=g, eps=1e-5, out_f32=True)
    assert rel_l2(a, b) < 1e-5
    assert within_one_ulp(ops.dec_proj(A, None, W8=q, E8=e, R=R), ops.dec_proj(A, wt, R=R))
    Wg = rnd(2 * 256, K, dtype=BF, seed=35, scale=K ** -0.5)
    qg, eg, wgt = fp8_weights(Wg)
    assert within_one_ulp(ops.dec_proj(A, None, mode=1, norm_w=g, eps=1e-5, W8=qg, E8=eg), ops.dec_proj(A, wgt, mode=1, norm_w=g, eps=1e-5))


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_dec_proj_fp8_refusals(dev):
    K, N = 256, 64
    A, W = rnd(4, K, dtype=BF, seed=1), rnd(N, K, dtype=BF, seed=2)
    q, e, _ = fp8_weights(W)
    with pytest.raises(ValueError):
        ops.dec_proj(A, None, W8=q, E8=None)                                      # exponents missing
    with pytest.raises(ValueError):
        ops.dec_proj(A[:, :192], None, W8=q[:, :192], E8=e[:, :6])               # K % 128
    flat = torch.zeros(N * K + 16, device=dev, dtype=torch.uint8)
    bad = flat[1:1 + N * K].view(N, K)
    bad.copy_(q)
    with pytest.raises(ValueError):
        ops.dec_proj(A, None, W8=bad, E8=e)                                       # misaligned codes
    assert torch.equal(ops.dec_proj(A, None, W8=flat[:N * K].view(N, K).copy_(q), E8=e, out_f32=True),
                       ops.dec_proj(A, None, W8=q, E8=e, out_f32=True))           # the same bytes at an aligned address run


# ------------------------------------------------------------------------------------------------ 5. token step
from dequant_weights import PROJ, dequantised  # noqa: E402,F401  (host code: tests/dequant_weights.py; other test files import it from here)


def _sd(hidden, heads, kvh, layers, ffn, vocab, seed=5):
    g = torch.Generator().manual_seed(seed)
    dkv = kvh * (hidden // heads)
    sd = {"model.embed_tokens.weight": torch.randn(vocab, hidden, generator=g) * 0.5, "model.norm.weight": 1 + 0.1 * torch.randn(hidden, generator=g),
          "lm_head.weight": torch.randn(vocab, hidden, generator=g) * hidden ** -0.5}
    for i in range(layers):
        p = f"model.layers.{i}."
        for nm, (o, k) in {"self_attn.q_proj": (hidden, hidden), "self_attn.k_proj": (dkv, hidden), "self_attn.v_proj": (dkv, hidden),
                           "self_attn.o_proj": (hidden, hidden), "mlp.gate_proj": (ffn, hidden), "mlp.up_proj": (ffn, hidden),
                           "mlp.down_proj": (hidden, ffn)}.items():
            sd[p + nm + ".weight"] = torch.randn(o, k, generator=g) * k ** -0.5
        sd[p + "input_layernorm.weight"] = 1 + 0.1 * torch.randn(hidden, generator=g)
        sd[p + "post_attention_layernorm.weight"] = 1 + 0.1 * torch.randn(hidden, generator=g)
    return sd


@pytest.fixture(scope="module")
def models():
    """The golden tiny model (with its adapters) and a 2-layer 4096-wide grouped-query model (Mistral-7B's attention widths)."""
    from avllm.arch import LlamaCfg
    from oracle import weights as Wt
    oc = Wt.tiny()
    W = Wt.all_weights(oc, 0, lora_b_std=0.05)
    big = LlamaCfg(4096, 32, 2, 2816, 2048)
    big.kv_heads = 8
    return {"tiny": (W["llama"], LlamaCfg(**vars(oc.llama)), W["lora"]), "gqa4096": (_sd(4096, 32, 8, 2, 2816, 2048), big, None)}


def _engines(dev, sd, cfg, lora_sd, with_lora):
    from avllm.arch import LoraCfg
    from avllm.engine import LlamaEngine
    lc = LoraCfg(16, 32.0) if with_lora else None
    if with_lora and lora_sd is None:
        g = torch.Generator().manual_seed(9)
        dkv = (cfg.kv_heads or cfg.heads) * (cfg.hidden // cfg.heads)
        lora_sd = {}
        for i in range(cfg.layers):
            for nm, do in (("q_proj", cfg.hidden), ("k_proj", dkv), ("v_proj", dkv), ("o_proj", cfg.hidden)):
                lora_sd[f"layers.{i}.{nm}.lora_A"] = torch.randn(16, cfg.hidden, generator=g) * cfg.hidden ** -0.5
                lora_sd[f"layers.{i}.{nm}.lora_B"] = torch.randn(do, 16, generator=g) * 0.05
    ls = lora_sd if with_lora else None
    e8 = LlamaEngine(sd, cfg, lc, ls, dtype=BF, device=dev, training=False, decode_fp8=True)
    et = LlamaEngine(dequantised(sd), cfg, lc, ls, dtype=BF, device=dev, training=False)
    e16 = LlamaEngine(sd, cfg, lc, ls, dtype=BF, device=dev, training=False)
    return e8, et, e16


@pytest.mark.parametrize("name", ["tiny", "gqa4096"])
@pytest.mark.parametrize("with_lora", [False, True])
def test_token_step_fp8_matches_bf16_step_on_dequantised_weights(dev, models, name, with_lora):
    sd, cfg, lora_sd = models[name]
    e8, et, e16 = _engines(dev, sd, cfg, lora_sd, with_lora)
    assert e8.decode_streams_fp8(1) and e8.decode_streams_fp8(16) and not e8.decode_streams_fp8(17)
    assert not et.decode_streams_fp8(8) and e8.decode_is_fused(16) == et.decode_is_fused(16)
    assert e8.streamed_weight_bytes(8) < 0.52 * e8.frozen_weight_bytes() and e8.streamed_weight_bytes(17) == e8.frozen_weight_bytes()
    S, new = 21, 3
    for B in (1, 8, 16):
        g = torch.Generator(device=dev).manual_seed(B)
        ids = torch.randint(0, cfg.vocab, (B, S + new), generator=g, device=dev)
        x = ops.embedding(e8.embed, ids.reshape(-1).contiguous()).view(B, S + new, cfg.hidden)
        kc, vc = e8.alloc_cache(B, S + new + 2)
        e8.prefill(x[:, :S].contiguous(), kc, vc)                # bf16 prefill on the original weights, shared by both token steps
        caches = [(kc.clone(), vc.clone()), (kc.clone(), vc.clone())]
        for use_dev in (False, True):
            pd = torch.zeros(1, device=dev, dtype=torch.int32) if use_dev else None
            k8, v8 = caches[0][0].clone(), caches[0][1].clone()
            kt, vt = caches[1][0].clone(), caches[1][1].clone()
            for t in range(new):
                tok = ids[:, S + t].contiguous()
                if use_dev:
                    a, b = e8.decode_step(tok, S, k8, v8, pos_dev=pd).clone(), et.decode_step(tok, S, kt, vt, pos_dev=pd).clone()
                    ops.L.check(ops.L.load().avllm_pos_advance(ops.L.ptr(pd), 1, ops.L.stream_ptr()))
                else:
                    a, b = e8.decode_step(tok, S + t, k8, v8).clone(), et.decode_step(tok, S + t, kt, vt).clone()
                # the fp32 grouping inside pairs of K-steps differs (dec_proj: f32 outputs within 1e-5, bf16 within one ulp), so some
                # bf16-rounded activations and cache rows land one ulp apart and later layers and steps carry that: measured 4e-4 (tiny) and
                # 4.6e-3 (4096 wide, random weights) -- bf16's own rounding noise, under half its bar (tests/bars.py, 2e-2)
                assert rel_l2(a, b) < 1e-2, (B, t, use_dev)
                top = b.topk(2, -1).values
                clear = (top[:, 0] - top[:, 1]) > 1e-2
                assert torch.equal(a.argmax(-1)[clear], b.argmax(-1)[clear]), (B, t, use_dev)
    # 17 rows: the general path on the bf16 matrices, bit for bit what an engine without decode_fp8 computes
    B = 17
    ids = torch.randint(0, cfg.vocab, (B, S + 1), generator=torch.Generator(device=dev).manual_seed(17), device=dev)
    x = ops.embedding(e8.embed, ids.reshape(-1).contiguous()).view(B, S + 1, cfg.hidden)
    outs = []
    for e in (e8, e16):
        kc, vc = e.alloc_cache(B, S + 2)
        e.prefill(x[:, :S].contiguous(), kc, vc)
        outs.append(e.decode_step(ids[:, S].contiguous(), S, kc, vc).clone())
    assert torch.equal(outs[0], outs[1])


def test_token_step_fp8_refused_without_images(dev, models):
    """check_llama refuses decode_fp8 without the codes / exponents: the step raises instead of reading NULL."""
    sd, cfg, _ = models["tiny"]
    e8, _, _ = _engines(dev, sd, cfg, None, False)
    B = 2
    kc, vc = e8.alloc_cache(B, 4)
    saved = e8.layers[1].egu8
    e8.layers[1].egu8 = None
    try:
        assert not e8.decode_streams_fp8(B)
        with pytest.raises(ValueError):
            e8.decode_step(torch.zeros(B, dtype=torch.int64, device=dev), 0, kc, vc)
    finally:
        e8.layers[1].egu8 = saved
    assert e8.decode_streams_fp8(B)
