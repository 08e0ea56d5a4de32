"""CPU: how model_type qwen3 decides the per-head q/k norms (from a checkpoint directory and from a config object), what is still refused,
that the synthetic weights of every other model are what they always were, that the g13 fixtures are what their recipe writes, and that the
float64 restatements of the two kernels (tests/refs64_qk_norm.py) are torch.autograd's answer and reachable in fp32 within tests/bars_qk_norm.py."""
import json
import os

import numpy as np
import pytest
import torch

import bars_qk_norm as QB
import qwen3_weights as QW
import refs64_qk_norm as R
from avllm import arch

QWEN3 = {"model_type": "qwen3", "architectures": ["Qwen3ForCausalLM"], "hidden_size": 4096, "num_attention_heads": 32, "num_key_value_heads": 8,
         "head_dim": 128, "num_hidden_layers": 36, "intermediate_size": 12288, "vocab_size": 151936, "rms_norm_eps": 1e-6, "rope_theta": 1000000.0,
         "attention_bias": False, "use_sliding_window": False, "sliding_window": None, "max_window_layers": 36, "tie_word_embeddings": False}


def cfg_of(tmp_path, c):
    (tmp_path / "config.json").write_text(json.dumps(c))
    return arch._cfg_from_hf_dir(str(tmp_path), "llama")


# ------------------------------------------------------------------------------------------------ configuration
def test_qwen3_config_has_qk_norm(tmp_path):
    c = cfg_of(tmp_path, QWEN3)
    assert c.qk_norm and not c.qkv_bias and not c.o_bias
    assert (c.hidden, c.heads, c.kv_heads, c.layers, c.ffn, c.vocab, c.eps, c.theta, c.head_dim) == (4096, 32, 8, 36, 12288, 151936, 1e-6, 1e6, 128)
    for hidden, heads in ((2048, 16), (5120, 40)):                      # 1.7B, 14B
        assert cfg_of(tmp_path, dict(QWEN3, hidden_size=hidden, num_attention_heads=heads)).qk_norm


def test_only_the_exact_model_type_enables_it(tmp_path):
    assert not cfg_of(tmp_path, dict(QWEN3, model_type="qwen3_moe")).qk_norm
    assert not cfg_of(tmp_path, dict(QWEN3, model_type="qwen2")).qk_norm
    assert not cfg_of(tmp_path, dict(QWEN3, model_type="llama")).qk_norm
    assert not arch.LlamaCfg().qk_norm and arch.LlamaCfg(64, 2, 3, 128, 64) == arch.LlamaCfg(64, 2, 3, 128, 64, qk_norm=False)
    assert not any(c.qk_norm for c in arch.LLAMA.values())


def test_qwen3_with_another_head_dim_is_still_refused(tmp_path):
    for hidden, heads in ((1024, 16), (2560, 32), (5120, 64)):          # 0.6B, 4B, 32B: head_dim 128 != hidden / heads
        with pytest.raises(NotImplementedError, match="head_dim"):
            cfg_of(tmp_path, dict(QWEN3, hidden_size=hidden, num_attention_heads=heads))
    with pytest.raises(NotImplementedError, match="sliding"):
        cfg_of(tmp_path, dict(QWEN3, use_sliding_window=True))


def test_provided_config_objects_resolve_the_same_way():
    tf = pytest.importorskip("transformers")
    flag = lambda hc: arch._qk_norm(lambda name, default: getattr(hc, name, default))
    assert flag(tf.Qwen3Config()) and not flag(tf.Qwen2Config()) and not flag(tf.LlamaConfig())
    assert not flag(tf.Qwen3MoeConfig())
    c = QW.CASES["a"]
    hc = tf.Qwen3Config(**{k: v for k, v in QW.hf_config_dict(c).items() if k not in ("model_type", "architectures")})
    prov = type("P", (), {"config": hc, "state_dict": lambda self: {}})()
    cfg, _ = arch.resolve_arch(None, "tiny", "base-patch16", None, {"whisper": {}, "clip": {}, "llama": {}}, 0, 8, 16, False, prov, None, None, "cpu",
                               torch.float32)
    assert cfg.llama == QW.llama_cfg(c) and cfg.llama.qk_norm
    hc.head_dim = 64                                                    # != 512 / 4
    with pytest.raises(NotImplementedError, match="head_dim"):
        arch.resolve_arch(None, "tiny", "base-patch16", None, {"whisper": {}, "clip": {}, "llama": {}}, 0, 8, 16, False, prov, None, None, "cpu", torch.float32)


# ------------------------------------------------------------------------------------------------ keys
def test_norm_keys_and_config_must_agree():
    c = QW.CASES["a"]
    on, off = QW.llama_cfg(c), QW.llama_cfg(c, qk_norm=False)
    sd = {k: torch.zeros(1) for k in QW.weights(c)[0]}
    arch.check_llama_keys(sd, on)
    arch.check_llama_keys(QW.without_norms(sd), off)
    for nm in ("q_norm", "k_norm"):
        key = f"model.layers.1.self_attn.{nm}.weight"
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            arch.check_llama_keys({k: v for k, v in sd.items() if k != key}, on)
        with pytest.raises(NotImplementedError, match="Qwen3.*does not declare"):
            arch.check_llama_keys(dict(QW.without_norms(sd), **{key: torch.zeros(1)}), off)
    with pytest.raises(NotImplementedError, match="MLP bias"):
        arch.check_llama_keys(dict(sd, **{"model.layers.0.mlp.up_proj.bias": torch.zeros(1)}), on)
    with pytest.raises(ValueError, match="q_proj.bias is present"):
        arch.check_llama_keys(dict(sd, **{"model.layers.0.self_attn.q_proj.bias": torch.zeros(1)}), on)


def test_synthetic_norms_come_after_every_other_draw():
    for extra_bias in (False, True):
        base = arch.LlamaCfg(128, 2, 2, 256, 96, 1e-6, 1e6, 1, (), extra_bias, False)
        qk = arch.LlamaCfg(128, 2, 2, 256, 96, 1e-6, 1e6, 1, (), extra_bias, False, True)
        a, b = arch.synth_llama(base, "cpu", torch.float32, 0), arch.synth_llama(qk, "cpu", torch.float32, 0)
        assert all(torch.equal(a[k], b[k]) for k in a)
        extra = sorted(set(b) - set(a))
        assert len(extra) == 2 * qk.layers and all(k.endswith(QW.NORM_KEYS) and b[k].shape == (64,) for k in extra)
        assert 0.8 < float(torch.stack([b[k] for k in extra]).mean()) < 1.2 and 0.05 < float(torch.stack([b[k] for k in extra]).std()) < 0.15
        arch.check_llama_keys(b, qk)
        with pytest.raises(NotImplementedError, match="Qwen3"):
            arch.check_llama_keys(b, base)


def test_config_only_directory_gives_a_seeded_model(tmp_path):
    """A directory with nothing but config.json (model_type qwen3) + synthetic_weights=True: a seeded model of that shape, norms included."""
    c = QW.CASES["a"]
    (tmp_path / "config.json").write_text(json.dumps(QW.hf_config_dict(c)))
    cfg, W = arch.resolve_arch(str(tmp_path), "tiny", "base-patch16", None, {"whisper": {}, "clip": {}}, 3, 8, 16, False, None, None, None, "cpu",
                               torch.float32, synthetic_weights=True)
    assert cfg.llama == QW.llama_cfg(c)
    arch.check_llama_keys(W["llama"], cfg.llama)
    assert W["llama"]["model.layers.1.self_attn.k_norm.weight"].shape == (128,)


# ------------------------------------------------------------------------------------------------ fixture
@pytest.mark.parametrize("case", ["a", "b"])
def test_fixture_is_what_the_recipe_writes(golden_dir, case):
    pytest.importorskip("transformers")
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(golden_dir), "..", "tools"))
    import make_golden_qwen3 as mk
    c = QW.CASES[case]
    path = os.path.join(golden_dir, QW.golden_name(c))
    assert os.path.getsize(path) < 1000000
    gold = np.load(path)
    arrays, margin = mk.run_case(c)
    assert margin >= mk.MARGIN
    assert np.abs(arrays["logits"] - gold[f"{case}.logits"]).max() <= 1e-5
    assert np.abs(arrays["step_logits"] - gold[f"{case}.step_logits"]).max() <= 1e-5
    assert np.array_equal(arrays["tokens"], gold[f"{case}.tokens"]) and np.array_equal(arrays["inputs_embeds"], gold[f"{case}.inputs_embeds"])
    assert abs(float(arrays["loss"]) - float(gold[f"{case}.loss"])) <= 1e-5
    assert sorted(f"{case}.{k}" for k in arrays) == sorted(gold.files)


# ------------------------------------------------------------------------------------------------ restatements and bars
def _case(fam, geo, M, T, dtype):
    H, Hkv, hd = geo
    x, (wq, wk) = R.inputs(fam, M, H, Hkv, hd, dtype), R.weights(fam, hd, dtype)
    return x, wq, wk, R.table(T, hd, 0 if T > 1 else 1000)


@pytest.mark.parametrize("geo", R.GEOMETRY)
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_restatements_are_autograds_answer(fam, geo):
    H, Hkv, hd = geo
    NQK, M = H + Hkv, 6
    x, wq, wk, tab = _case(fam, geo, M, 3, torch.float32)
    X = x[:, :NQK * hd].double().reshape(M, NQK, hd).requires_grad_(True)
    W = torch.cat([wq.double()[None].expand(H, -1), wk.double()[None].expand(Hkv, -1)], 0)
    var = X.pow(2).mean(-1, keepdim=True)                               # Qwen3RMSNorm.forward
    y = W * (X * torch.rsqrt(var + R.EPS))
    t = torch.arange(M) % 3
    cos = torch.cat([tab[t, :, 0], tab[t, :, 0]], -1).double()[:, None, :]      # apply_rotary_pos_emb: q cos + rotate_half(q) sin
    sin = torch.cat([tab[t, :, 1], tab[t, :, 1]], -1).double()[:, None, :]
    rot = y * cos + torch.cat([-y[..., hd // 2:], y[..., :hd // 2]], -1) * sin
    ref = R.fwd64(x, H, Hkv, hd, wq, wk, R.EPS, tab)
    rot = rot.detach()
    assert float((ref.out - rot.reshape(M, -1)).abs().max()) <= 1e-12 * max(1.0, float(rot.abs().max()))
    dy = R.inputs(fam, M, H, Hkv, hd, torch.float32, "dy")
    y.backward(dy[:, :NQK * hd].double().reshape(M, NQK, hd))
    got = R.bwd64(dy, x[:, :NQK * hd], ref.rstd, H, Hkv, hd, wq, wk)
    assert float((got.dx - X.grad.reshape(M, -1)).abs().max()) <= 1e-12 * max(1.0, float(X.grad.abs().max()))
    if fam == "locate":                                                 # q's and k's vectors are disjoint and distinct per index
        assert len(set(wq.tolist()) | set(wk.tolist())) == 2 * hd


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("geo", R.GEOMETRY)
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_bars_are_reachable_in_fp32(fam, geo, dtype):
    """The restatement evaluated in float32 (then rounded once for a bf16 buffer) is inside every bar: the bars can be met by the reference
    arithmetic alone."""
    H, Hkv, hd = geo
    NQK, M, rounded = H + Hkv, 48, dtype == torch.bfloat16
    x, wq, wk, tab = _case(fam, geo, M, 24, dtype)
    ref, f32 = R.fwd64(x, H, Hkv, hd, wq, wk, R.EPS, tab), R.fwd64(x, H, Hkv, hd, wq, wk, R.EPS, tab, torch.float32)
    out32 = R.stored(f32.out, dtype).double()
    assert bool(((out32 - ref.out).abs() <= QB.fwd_bar(ref, rounded)).all())
    assert bool(((f32.rstd.double() - ref.rstd).abs() <= QB.rstd_bar(ref, not rounded)).all())
    pre, rstd = x[:, :NQK * hd], f32.rstd
    dy = R.inputs(fam, M, H, Hkv, hd, dtype, "dy")
    b64, b32 = R.bwd64(dy, pre, rstd, H, Hkv, hd, wq, wk), R.bwd64(dy, pre, rstd, H, Hkv, hd, wq, wk, torch.float32)
    assert bool(((R.stored(b32.dx, dtype).double() - b64.dx).abs() <= QB.bwd_bar(b64, b32, rounded)).all())
    dyr, w1, _ = R.radial(pre, rstd, H, Hkv, hd)
    r64, r32 = R.bwd64(dyr, pre, rstd, H, Hkv, hd, w1, w1), R.bwd64(dyr, pre, rstd, H, Hkv, hd, w1, w1, torch.float32)
    bar = QB.radial_bar(r64, hd, rounded)
    assert bool(((R.stored(r32.dx, dtype).double() - r64.dx).abs() <= bar).all())
    if fam != "tiny":                                                   # the exact result is eps-small: the bar is an absolute bound, far under |g| rstd
        assert float(r64.dx.abs().max()) < 1e-4 * float((r64.g.abs() * r64.rstd[..., None]).max())
        assert float(bar.max()) < 1e-3 * float((r64.g.abs() * r64.rstd[..., None]).max())
