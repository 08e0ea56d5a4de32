"""Weight-only fp4 token step: avllm_mx4_quantize (OCP MXFP4 codes + E8M0 exponents), the fp4 weight form of avllm_dec_proj and the engine's
decode_fp4 mode.  Numerics definition, as for fp8: the fp4 form computes what the bf16 form computes on W~ = dequantize(codes, exponents),
which is an ordinary (exactly representable) bf16 weight set; only the fp32 summation order inside a 128-column group of K-steps differs.
Every comparison is against W~, never against W: the format's own error (about 11.5 % on Gaussian weights) is not what is tested here.

The projection tests feed codes made on the CPU by tests/mxfp4_ref.py, so the quantiser and the kernel's dequantiser cannot be wrong
together (the nibble order among it)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mxfp4_ref as mx4  # noqa: E402
from avllm import ops  # noqa: E402
from bars import rel_l2  # noqa: E402
from oracle import mxfp8  # noqa: E402
from test_decode_fp8_gpu import PROJ, _rope, _rot, models, rms, within_one_ulp  # noqa: E402,F401
from test_ops_gpu import rnd  # noqa: E402

BF = torch.bfloat16
_CACHE = {}


def fp4_weights(N, K, seed):
    """(packed codes, biased exponents) made on the CPU by mxfp4_ref and uploaded, and W~ as a bf16 tensor (exact).  One per (N, K, seed)."""
    key = (N, K, seed)
    if key not in _CACHE:
        W = rnd(N, K, dtype=BF, seed=seed, scale=K ** -0.5, dev="cpu").float()
        codes, e = mx4.quantize(W)
        wt = mx4.dequantize(codes, e)
        wt16 = wt.to(BF)
        assert torch.equal(wt16.float(), wt)                  # W~ is a bf16 weight set
        _CACHE[key] = (mx4.pack(codes).cuda(), (e + 127).to(torch.uint8).cuda(), wt16.cuda())
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ 1. quantiser
@pytest.mark.parametrize("R,K", [(16, 128), (16, 11008), (4608, 4096), (32000, 128)])
def test_mx4_quantize_matches_the_cpu_rule(dev, R, K):
    W = rnd(R, K, dtype=BF, seed=7, scale=K ** -0.5)
    W[:3, :32] = 0                                        # an all-zero block: exponent -127 (biased 0), codes 0
    q, e = ops.mx4_quantize(W)
    assert q.shape == (R, K // 2) and q.dtype == torch.uint8 and e.shape == (R, K // 32) and e.dtype == torch.uint8
    codes, ex = mx4.quantize(W.cpu().float())
    assert torch.equal(e.cpu().to(torch.int32), ex + 127)
    assert torch.equal(q.cpu(), mx4.pack(codes))
    qf, ef = ops.mx4_quantize(W.float())                  # f32 input: the same image
    assert torch.equal(qf, q) and torch.equal(ef, e)


def test_mx4_quantize_ties_and_saturation(dev):
    """The rounding table of the format on the device: ties to the even code, saturation at +-6, the sign in bit 3."""
    vals = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0, 0.3, 1.3, 2.6, 5.1, 6.0, 0.0]
    x = torch.zeros(2, 32)
    x[:, 0] = 7.5                                         # amax 7.5: exponent 0, scale 1
    x[0, 1:1 + len(vals)] = torch.tensor(vals)
    x[1, 1:1 + len(vals)] = -torch.tensor(vals)
    q, e = ops.mx4_quantize(x.cuda())
    codes, ex = mx4.quantize(x)
    assert e.cpu().tolist() == [[127], [127]]
    assert torch.equal(q.cpu(), mx4.pack(codes))
    assert mx4.unpack(q.cpu())[0, 1:9].tolist() == [0, 2, 2, 4, 4, 6, 6, 7]
    assert mx4.unpack(q.cpu())[1, 1:9].tolist() == [8, 10, 10, 12, 12, 14, 14, 15]


# ------------------------------------------------------------------------------------------------ 2. dec_proj fp4 (CPU-made codes) vs torch on W~
# K: one group (128), an uneven deal (1152: 2,1,1,..), odd / even group counts per wave (2944: 3 / 2; 4096: 4; 11008: 11 / 10), and 5120
# (5 groups per wave): with the ring of 4 (3 at M > 8) groups these reach every length of the straight-line tail, 1 .. 7 (1 .. 5)
@pytest.mark.parametrize("K", [128, 1152, 2944, 4096, 5120, 11008])
@pytest.mark.parametrize("M", [1, 4, 5, 8, 9, 16])
def test_dec_proj_fp4_plain_norm_residual(dev, M, K):
    N = 528
    A = rnd(M, K, dtype=BF, seed=1)
    R, g = rnd(M, N, dtype=BF, seed=3), (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=4)).to(BF)
    q, e, wt = fp4_weights(N, K, 2)
    ref = A.float() @ wt.float().t()
    assert rel_l2(ops.dec_proj(A, None, W4=q, E8=e, out_f32=True), ref) < 2e-3
    out = R.clone()
    ops.dec_proj(A, None, W4=q, E8=e, R=out, out=out)
    assert rel_l2(out, ref + R.float()) < 6e-3
    refn = rms(A, g, 1e-5) @ wt.float().t()
    assert rel_l2(ops.dec_proj(A, None, W4=q, E8=e, norm_w=g, eps=1e-5, out_f32=True), refn) < 6e-3
    rows = rnd(4 * M, K, dtype=BF, seed=5)
    assert rel_l2(ops.dec_proj(rows[3::4], None, W4=q, E8=e, out_f32=True), rows[3::4].float() @ wt.float().t()) < 2e-3


def test_dec_proj_fp4_uses_each_blocks_own_exponent(dev):
    """Rows whose four blocks of a group carry four different exponents, and a one-hot activation per block: a wrong scale byte or a wrong
    nibble shows as a wrong value, not as noise under a tolerance."""
    N, K, M = 16, 256, 4
    W = torch.zeros(N, K)
    for b in range(K // 32):
        W[:, 32 * b:32 * b + 32] = (torch.arange(32) % 7 - 3).float() * 2.0 ** (b - 3) * (1.0 - 2.0 * (torch.arange(N) % 2)).float()[:, None]
    W[:, 1::2] *= 0.5                                     # odd elements differ from their even neighbours
    codes, e = mx4.quantize(W)
    wt = mx4.dequantize(codes, e)
    assert torch.equal(wt, W) and len(set(e[0].tolist())) == K // 32      # on the grid as written; every block its own exponent
    q, ex = mx4.pack(codes).cuda(), (e + 127).to(torch.uint8).cuda()
    A = torch.zeros(M, K)
    for m in range(M):
        A[m, 37 * m + 1::64] = 1.0                        # picks single elements of different blocks, odd and even ones
    out = ops.dec_proj(A.to(BF).cuda(), None, W4=q, E8=ex, out_f32=True)
    assert torch.equal(out.cpu(), A @ wt.t())             # sums of a few exactly representable values: exact


# ------------------------------------------------------------------------------------------------ 5. forced activation-load forms
@pytest.mark.parametrize("M,al", [(1, "2"), (1, "4"), (3, "4"), (4, "2"), (5, "4"), (8, "4")])
def test_dec_proj_fp4_activation_load_forms(dev, M, al):
    """The forced wider activation-load forms (AVLLM_DEC_AL) give bit-identical sums: the same elements meet in the same order."""
    K = 2944
    A = rnd(M, K, dtype=BF, seed=1)
    g = (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=4)).to(BF)
    q, e, wt = fp4_weights(528, K, 2)
    want = ops.dec_proj(A, None, W4=q, E8=e, out_f32=True), ops.dec_proj(A, None, W4=q, E8=e, norm_w=g, eps=1e-5, out_f32=True)
    with ops.L.knob("DEC_AL", int(al)):
        got = ops.dec_proj(A, None, W4=q, E8=e, out_f32=True), ops.dec_proj(A, None, W4=q, E8=e, norm_w=g, eps=1e-5, out_f32=True)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    assert rel_l2(want[0], A.float() @ wt.float().t()) < 2e-3
    assert rel_l2(want[1], rms(A, g, 1e-5) @ wt.float().t()) < 6e-3


# ------------------------------------------------------------------------------------------------ 3. SwiGLU, q|k|v, adapters
@pytest.mark.parametrize("M,K,F", [(1, 256, 64), (8, 4096, 11008), (16, 1152, 520), (5, 11008, 128)])
def test_dec_proj_fp4_swiglu(dev, M, K, F):
    A = rnd(M, K, dtype=BF, seed=11)
    g = (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=13)).to(BF)
    q, e, wt = fp4_weights(2 * F, K, 12)
    xn = rms(A, g, 1e-6)
    gate, up = xn @ wt[:F].float().t(), xn @ wt[F:].float().t()
    out = ops.dec_proj(A, None, mode=1, norm_w=g, eps=1e-6, W4=q, E8=e)
    assert out.shape == (M, F) and rel_l2(out, torch.nn.functional.silu(gate) * up) < 8e-3


@pytest.mark.parametrize("M,heads,kvh,hd,K", [(1, 4, 4, 128, 128), (8, 4, 2, 64, 256), (16, 8, 2, 128, 1024), (4, 32, 8, 128, 4096)])
def test_dec_proj_fp4_qkv_rope_cache(dev, M, heads, kvh, hd, K):
    dq, dkv, Tmax, pos = heads * hd, kvh * hd, 9, 5
    A = rnd(M, K, dtype=BF, seed=21)
    g = (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=23)).to(BF)
    q4, e4, wt = fp4_weights(dq + 2 * dkv, K, 22)
    ang, rope = _rope(dev, hd, pos)
    y = rms(A, g, 1e-5) @ wt.float().t()
    for use_dev in (False, True):
        kc = torch.full((M, Tmax, dkv), 7.0, device=dev, dtype=BF)
        vc = torch.full((M, Tmax, dkv), -7.0, device=dev, dtype=BF)
        pd = torch.tensor([3], device=dev, dtype=torch.int32) if use_dev else None
        q = ops.dec_proj(A, None, mode=2, norm_w=g, eps=1e-5, rope=rope, kc=kc, vc=vc, pos=pos - (3 if use_dev else 0), pos_dev=pd, dq=dq, dkv=dkv,
                         hd=hd, W4=q4, E8=e4)
        assert rel_l2(q, _rot(y[:, :dq], ang, M, heads, hd)) < 8e-3
        assert rel_l2(kc[:, pos], _rot(y[:, dq:dq + dkv], ang, M, kvh, hd)) < 8e-3
        assert rel_l2(vc[:, pos], y[:, dq + dkv:]) < 8e-3
        keep = [t for t in range(Tmax) if t != pos]
        assert (kc[:, keep] == 7.0).all() and (vc[:, keep] == -7.0).all()


@pytest.mark.parametrize("M,r", [(1, 16), (5, 8), (16, 4)])
def test_dec_proj_fp4_adapter_side_term(dev, M, r):
    """peft lora.Linear on the fp4 token step: the base product streams codes, the rank-side products and B images stay bf16."""
    K, scale = 1152, 2.0
    g = (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=43)).to(BF)
    A = rnd(M, K, dtype=BF, seed=41)
    N = 528
    q4, e4, wt = fp4_weights(N, K, 42)
    Ap = torch.zeros(64, K, device=dev, dtype=BF); Ap[:r] = rnd(r, K, dtype=BF, seed=44, scale=K ** -0.5)
    Bp = torch.zeros(N, 64, device=dev, dtype=BF); Bp[:, :r] = rnd(N, r, dtype=BF, seed=45, scale=0.3)
    R = rnd(M, N, dtype=BF, seed=46)
    t = torch.zeros(M, 256, device=dev, dtype=torch.float32)
    ops.dec_proj(A, Ap[:16], out=t[:, 192:208], out_f32=True)
    ref_t = A.float() @ Ap[:16].float().t()
    out = ops.dec_proj(A, None, W4=q4, E8=e4, R=R, lora_t=t[:, 192:], lora_b=[Bp], lora_r=r, lora_scale=scale, out_f32=True)
    ref = A.float() @ wt.float().t() + R.float() + scale * (ref_t[:, :r] @ Bp[:, :r].float().t())
    assert rel_l2(out, ref) < 3e-3
    # q|k|v with norm + RoPE + cache and the three adapters
    heads, kvh, hd, Tmax, pos = 4, 2, 64, 6, 3
    dq, dkv = heads * hd, kvh * hd
    q4, e4, wqt = fp4_weights(dq + 2 * dkv, K, 47)
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
                     lora_t=t, lora_b=Bs, lora_r=r, lora_scale=scale, W4=q4, E8=e4)
    assert rel_l2(q, _rot(y[:, :dq], ang, M, heads, hd)) < 8e-3
    assert rel_l2(kc[:, pos], _rot(y[:, dq:dq + dkv], ang, M, kvh, hd)) < 8e-3
    assert rel_l2(vc[:, pos], y[:, dq + dkv:]) < 8e-3


# ------------------------------------------------------------------------------------------------ 4. same products as bf16 on W~
@pytest.mark.parametrize("K", [128, 4096, 5120, 11008])
@pytest.mark.parametrize("M", [1, 5, 8, 16])
def test_dec_proj_fp4_matches_bf16_form_on_dequantised_weights(dev, M, K):
    """fp4 form vs the bf16 form over W~: the products are identical, only the fp32 grouping inside a 128-column group differs.  The bars
    are the project's figures for "same products, other fp32 grouping" (the fp8 form's); measured on f32 outputs: <= 1.3e-7."""
    N = 528
    A = rnd(M, K, dtype=BF, seed=31)
    R, g = rnd(M, N, dtype=BF, seed=33), (1.0 + 0.1 * rnd(K, dtype=torch.float32, seed=34)).to(BF)
    q, e, wt = fp4_weights(N, K, 32)
    a = ops.dec_proj(A, None, W4=q, E8=e, norm_w=g, eps=1e-5, out_f32=True)
    b = ops.dec_proj(A, wt, norm_w=g, eps=1e-5, out_f32=True)
    print(f"fp4 vs bf16 form on W~, M={M} K={K}: rel_l2 {rel_l2(a, b):.3e}")
    assert rel_l2(a, b) < 1e-5
    assert within_one_ulp(ops.dec_proj(A, None, W4=q, E8=e, R=R), ops.dec_proj(A, wt, R=R))
    qg, eg, wgt = fp4_weights(2 * 256, K, 35)
    assert within_one_ulp(ops.dec_proj(A, None, mode=1, norm_w=g, eps=1e-5, W4=qg, E8=eg), ops.dec_proj(A, wgt, mode=1, norm_w=g, eps=1e-5))


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_dec_proj_fp4_refusals(dev):
    K, N = 256, 64
    A = rnd(4, K, dtype=BF, seed=1)
    q, e, _ = fp4_weights(N, K, 2)
    with pytest.raises(ValueError):
        ops.dec_proj(A, None, W4=q, E8=None)                                      # exponents missing
    with pytest.raises(ValueError):
        ops.dec_proj(A[:, :192], None, W4=q[:, :96], E8=e[:, :6])                # K % 128
    flat = torch.zeros(N * K // 2 + 16, device=dev, dtype=torch.uint8)
    bad = flat[1:1 + N * K // 2].view(N, K // 2)
    bad.copy_(q)
    with pytest.raises(ValueError):
        ops.dec_proj(A, None, W4=bad, E8=e)                                       # misaligned codes
    q8, e8 = ops.mx_quantize(rnd(N, K, dtype=BF, seed=2), 2)
    with pytest.raises(ValueError):
        ops.dec_proj(A, None, W4=q, W8=q8, E8=e)                                  # two weight forms at once
    assert torch.equal(ops.dec_proj(A, None, W4=flat[:N * K // 2].view(N, K // 2).copy_(q), E8=e, out_f32=True),
                       ops.dec_proj(A, None, W4=q, E8=e, out_f32=True))           # the same bytes at an aligned address run


# ------------------------------------------------------------------------------------------------ 7. token step
from dequant_weights import dequantised4  # noqa: E402,F401  (host code: tests/dequant_weights.py; other test files import it from here)


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
    e4 = LlamaEngine(sd, cfg, lc, ls, dtype=BF, device=dev, training=False, decode_fp4=True)
    et = LlamaEngine(dequantised4(sd), cfg, lc, ls, dtype=BF, device=dev, training=False)
    e16 = LlamaEngine(sd, cfg, lc, ls, dtype=BF, device=dev, training=False)
    return e4, et, e16


def _fp4_step_bytes(cfg):
    d, f, hd = cfg.hidden, cfg.ffn, cfg.hidden // cfg.heads
    dkv = (getattr(cfg, "kv_heads", 0) or cfg.heads) * hd
    proj = [(d + 2 * dkv, d), (d, d), (2 * f, d), (d, f)]
    return cfg.layers * sum(n * k // 2 + n * k // 32 for n, k in proj) + cfg.vocab * d + cfg.vocab * d // 32


@pytest.mark.parametrize("name", ["tiny", "gqa4096"])
@pytest.mark.parametrize("with_lora", [False, True])
def test_token_step_fp4_matches_bf16_step_on_dequantised_weights(dev, models, name, with_lora):
    sd, cfg, lora_sd = models[name]
    e4, et, e16 = _engines(dev, sd, cfg, lora_sd, with_lora)
    assert e4.decode_streams_fp4(1) and e4.decode_streams_fp4(16) and not e4.decode_streams_fp4(17)
    assert not e4.decode_streams_fp8(8) and not et.decode_streams_fp4(8) and e4.decode_is_fused(16) == et.decode_is_fused(16)
    assert e4.streamed_weight_bytes(8) == _fp4_step_bytes(cfg) and e4.streamed_weight_bytes(17) == e4.frozen_weight_bytes()
    S, new = 21, 3
    for B in (1, 8, 16):
        g = torch.Generator(device=dev).manual_seed(B)
        ids = torch.randint(0, cfg.vocab, (B, S + new), generator=g, device=dev)
        x = ops.embedding(e4.embed, ids.reshape(-1).contiguous()).view(B, S + new, cfg.hidden)
        kc, vc = e4.alloc_cache(B, S + new + 2)
        e4.prefill(x[:, :S].contiguous(), kc, vc)                # bf16 prefill on the original weights, shared by both token steps
        for use_dev in (False, True):
            pd = torch.zeros(1, device=dev, dtype=torch.int32) if use_dev else None
            k4, v4 = kc.clone(), vc.clone()
            kt, vt = kc.clone(), vc.clone()
            for t in range(new):
                tok = ids[:, S + t].contiguous()
                if use_dev:
                    a, b = e4.decode_step(tok, S, k4, v4, pos_dev=pd).clone(), et.decode_step(tok, S, kt, vt, pos_dev=pd).clone()
                    ops.L.check(ops.L.load().avllm_pos_advance(ops.L.ptr(pd), 1, ops.L.stream_ptr()))
                else:
                    a, b = e4.decode_step(tok, S + t, k4, v4).clone(), et.decode_step(tok, S + t, kt, vt).clone()
                # same mechanism and bars as the fp8 step: identical products, another fp32 grouping, so some bf16-rounded activations and
                # cache rows land one ulp apart and later layers and steps carry that (measured: <= 8e-8 tiny, <= 2.2e-3 at 4096 wide)
                print(f"{name} lora={with_lora} B={B} t={t} dev={use_dev}: rel_l2 {rel_l2(a, b):.3e}")
                assert rel_l2(a, b) < 1e-2, (B, t, use_dev)
                top = b.topk(2, -1).values
                clear = (top[:, 0] - top[:, 1]) > 1e-2
                assert torch.equal(a.argmax(-1)[clear], b.argmax(-1)[clear]), (B, t, use_dev)
    # 17 rows: the general path on the bf16 matrices, bit for bit what an engine without decode_fp4 computes
    B = 17
    ids = torch.randint(0, cfg.vocab, (B, S + 1), generator=torch.Generator(device=dev).manual_seed(17), device=dev)
    x = ops.embedding(e4.embed, ids.reshape(-1).contiguous()).view(B, S + 1, cfg.hidden)
    outs = []
    for e in (e4, e16):
        kc, vc = e.alloc_cache(B, S + 2)
        e.prefill(x[:, :S].contiguous(), kc, vc)
        outs.append(e.decode_step(ids[:, S].contiguous(), S, kc, vc).clone())
    assert torch.equal(outs[0], outs[1])


def test_token_step_fp4_refused_without_images_or_with_fp8(dev, models):
    """check_llama refuses decode_fp4 without the codes / exponents, and together with decode_fp8: the step raises instead of reading NULL."""
    from avllm.engine import LlamaEngine
    sd, cfg, _ = models["tiny"]
    e4, _, _ = _engines(dev, sd, cfg, None, False)
    B = 2
    kc, vc = e4.alloc_cache(B, 4)
    tok = torch.zeros(B, dtype=torch.int64, device=dev)
    saved = e4.layers[1].egu4
    e4.layers[1].egu4 = None
    try:
        assert not e4.decode_streams_fp4(B)
        with pytest.raises(ValueError):
            e4.decode_step(tok, 0, kc, vc)
    finally:
        e4.layers[1].egu4 = saved
    assert e4.decode_streams_fp4(B)
    e4.desc.decode_fp8 = 1
    try:
        assert not e4.decode_streams_fp4(B) and not e4.decode_streams_fp8(B)
        with pytest.raises(ValueError):
            e4.decode_step(tok, 0, kc, vc)
    finally:
        e4.desc.decode_fp8 = 0
    e4.decode_step(tok, 0, kc, vc)
    with pytest.raises(ValueError):
        LlamaEngine(sd, cfg, None, None, dtype=BF, device=dev, training=False, decode_fp8=True, decode_fp4=True)
    with pytest.raises(ValueError):
        LlamaEngine(sd, cfg, None, None, dtype=torch.float32, device=dev, training=False, decode_fp4=True)
