"""CPU: how a checkpoint directory's config.json decides the attention biases (Qwen2: q, k, v; attention_bias: o as well), what is refused by name,
that bias-free synthetic weights are what they always were, and that the g12 fixture is what its recipe writes."""
import hashlib
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_bias_weights as AW
from avllm import arch

QWEN = {"model_type": "qwen2", "architectures": ["Qwen2ForCausalLM"], "hidden_size": 896, "num_attention_heads": 14, "num_key_value_heads": 2,
        "num_hidden_layers": 24, "intermediate_size": 4864, "vocab_size": 151936, "rms_norm_eps": 1e-6, "rope_theta": 1000000.0,
        "use_sliding_window": False, "sliding_window": 32768, "max_window_layers": 21, "tie_word_embeddings": True}
LLAMA = {"model_type": "llama", "hidden_size": 512, "num_attention_heads": 4, "num_key_value_heads": 2, "num_hidden_layers": 2,
         "intermediate_size": 1024, "vocab_size": 512, "rms_norm_eps": 1e-5, "rope_theta": 10000.0}


def case_with(c, **kw):
    """Case c of attn_bias_weights with some fields replaced."""
    return SimpleNamespace(**dict(vars(c), **kw))


def cfg_of(tmp_path, c):
    (tmp_path / "config.json").write_text(json.dumps(c))
    return arch._cfg_from_hf_dir(str(tmp_path), "llama")


def test_qwen2_config_has_qkv_bias(tmp_path):
    c = cfg_of(tmp_path, QWEN)
    assert (c.qkv_bias, c.o_bias) == (True, False)
    assert c.theta == 1e6 and c.eps == 1e-6 and (c.hidden, c.heads, c.kv_heads, c.layers, c.ffn, c.vocab) == (896, 14, 2, 24, 4864, 151936)
    t = arch.LLAMA["qwen2.5-0.5b"]                        # the table row is the same model
    assert c == t


def test_rope_parameters_spelling_of_the_same_config(tmp_path):
    q = {k: v for k, v in QWEN.items() if k != "rope_theta"}
    q["rope_parameters"] = {"rope_theta": 1000000.0, "rope_type": "default"}
    c = cfg_of(tmp_path, q)
    assert c.theta == 1e6 and c.qkv_bias and not c.o_bias and c.rope_scaling == ()


def test_llama_attention_bias_has_both(tmp_path):
    c = cfg_of(tmp_path, dict(LLAMA, attention_bias=True))
    assert (c.qkv_bias, c.o_bias) == (True, True)
    c = cfg_of(tmp_path, LLAMA)
    assert (c.qkv_bias, c.o_bias) == (False, False)
    c = cfg_of(tmp_path, dict(LLAMA, attention_bias=False))
    assert (c.qkv_bias, c.o_bias) == (False, False)


def test_table_rows_carry_the_bias():
    for name in ("qwen2.5-0.5b", "qwen2.5-1.5b", "qwen2.5-3b", "qwen2.5-7b"):
        c = arch._from_name("Qwen/" + name.replace("qwen", "Qwen").replace("b", "B"), arch.LLAMA, "llama")
        assert c is arch.LLAMA[name] and c.qkv_bias and not c.o_bias and c.theta == 1e6 and c.eps == 1e-6
        assert c.hidden % c.heads == 0 and c.head_dim == (64 if name == "qwen2.5-0.5b" else 128)
    for name, c in arch.LLAMA.items():
        assert c.qkv_bias == name.startswith("qwen") and not c.o_bias


def test_sliding_window_is_refused(tmp_path):
    with pytest.raises(NotImplementedError, match="sliding"):
        cfg_of(tmp_path, dict(QWEN, use_sliding_window=True))


def _keys(c):
    return {k: torch.zeros(1) for k in arch.synth_llama(AW.llama_cfg(c), "cpu", torch.float32, 0)}


def test_other_architectures_tensors_are_refused_by_name():
    c = AW.CASES["q"]
    cfg, sd = AW.llama_cfg(c), _keys(c)
    arch.check_llama_keys(sd, cfg)
    for nm in ("gate_proj", "up_proj", "down_proj"):
        with pytest.raises(NotImplementedError, match="MLP bias"):
            arch.check_llama_keys(dict(sd, **{f"model.layers.1.mlp.{nm}.bias": torch.zeros(1)}), cfg)
    for nm in ("q_norm", "k_norm"):
        with pytest.raises(NotImplementedError, match="Qwen3"):
            arch.check_llama_keys(dict(sd, **{f"model.layers.0.self_attn.{nm}.weight": torch.zeros(1)}), cfg)


def test_bias_keys_and_config_must_agree():
    q, l = AW.CASES["q"], AW.CASES["l"]
    plain = arch.LlamaCfg(896, 14, 2, 1152, 512, 1e-6, 1e6, 2)
    with pytest.raises(ValueError, match="q_proj.bias is present"):
        arch.check_llama_keys(_keys(q), plain)                                   # a Qwen checkpoint under a config that says no
    with pytest.raises(ValueError, match="q_proj.bias is missing"):
        arch.check_llama_keys(_keys(case_with(q, qkv_bias=False)), AW.llama_cfg(q))      # the converse
    with pytest.raises(ValueError, match="o_proj.bias is missing"):
        arch.check_llama_keys(_keys(case_with(l, o_bias=False)), AW.llama_cfg(l))
    with pytest.raises(ValueError, match="o_proj.bias is present"):
        arch.check_llama_keys(_keys(l), AW.llama_cfg(case_with(l, o_bias=False)))
    arch.check_llama_keys(_keys(l), AW.llama_cfg(l))
    arch.check_llama_keys(_keys(case_with(q, qkv_bias=False)), plain)


def _checksum(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().view(torch.uint8).numpy().tobytes())
    return len(sd), h.hexdigest()


def test_bias_free_synthetic_weights_are_unchanged():
    """sha256 over the sorted keys and bytes of synth_llama's output, recorded on the commit before the biases existed."""
    assert _checksum(arch.synth_llama(arch.LlamaCfg(128, 4, 2, 256, 96, 1e-5, 10000.0, 2), "cpu", torch.float32, 0)) == \
        (21, "83a65f833eeb5cf24326ba037bd5ac1d4ab10683b30c4e3d29be7daf70826ab3")
    assert _checksum(arch.synth_llama(arch.LlamaCfg(64, 2, 3, 128, 64), "cpu", torch.bfloat16, 5)) == \
        (30, "02763fdf06e8fca37a7842bfd61687f72368a5662a885c59f7db3f34e47b082d")


def test_synthetic_biases_come_after_every_other_draw():
    base = arch.LlamaCfg(128, 4, 2, 256, 96, 1e-5, 10000.0, 2)
    both = arch.LlamaCfg(128, 4, 2, 256, 96, 1e-5, 10000.0, 2, (), True, True)
    a, b = arch.synth_llama(base, "cpu", torch.float32, 0), arch.synth_llama(both, "cpu", torch.float32, 0)
    assert all(torch.equal(a[k], b[k]) for k in a)
    extra = sorted(set(b) - set(a))
    assert len(extra) == 8 and all(k.endswith("_proj.bias") for k in extra)
    assert b["model.layers.1.self_attn.k_proj.bias"].shape == (64,) and b["model.layers.0.self_attn.o_proj.bias"].shape == (128,)
    assert 0.2 < float(b["model.layers.0.self_attn.q_proj.bias"].std()) < 0.4
    arch.check_llama_keys(b, both)


@pytest.mark.parametrize("case", ["q", "l"])
def test_fixture_is_what_the_recipe_writes(golden_dir, case):
    pytest.importorskip("transformers")
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(golden_dir), "..", "tools"))
    import make_golden_qwen2 as mk
    c = AW.CASES[case]
    gold = np.load(os.path.join(golden_dir, AW.golden_name(c)))
    arrays, margin = mk.run_case(c)
    assert margin >= mk.MARGIN
    assert np.abs(arrays["logits"] - gold[f"{case}.logits"]).max() <= 1e-5
    assert np.abs(arrays["step_logits"] - gold[f"{case}.step_logits"]).max() <= 1e-5
    assert np.array_equal(arrays["tokens"], gold[f"{case}.tokens"]) and np.array_equal(arrays["inputs_embeds"], gold[f"{case}.inputs_embeds"])
    assert abs(float(arrays["loss"]) - float(gold[f"{case}.loss"])) <= 1e-5
    assert sorted(f"{case}.{k}" for k in arrays) == sorted(gold.files)


def test_provided_config_objects_resolve_the_same_way():
    """The `_provided_llm` branch reads the same three fields off a transformers config object."""
    tf = pytest.importorskip("transformers")
    flags = lambda hc: arch._attn_biases(lambda name, default: getattr(hc, name, default))
    assert flags(tf.Qwen2Config()) == (True, False)
    assert flags(tf.LlamaConfig(attention_bias=True)) == (True, True)
    assert flags(tf.LlamaConfig()) == (False, False)
    with pytest.raises(NotImplementedError, match="sliding"):
        flags(tf.Qwen2Config(use_sliding_window=True))
