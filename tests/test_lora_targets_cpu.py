"""CPU: the rules of lora_target_modules that need no HIP library -- parsing and refusals, the flat-buffer layout, the dropout-seed rule, the
peft key names -- and the control that ties tests/refs64_lora_mlp.py (the float64 reference of tests/test_lora_mlp_gpu.py) to the pinned oracle."""
import pytest
import torch

import refs64_lora_mlp as R
from avllm import arch as A
from oracle import avsr_oracle as O
from oracle import weights as Wt

ALL = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")


def test_parsing():
    assert A.LORA_MODULES == ALL and A.LORA_DEFAULT_TARGETS == ALL[:4] and A.LoraCfg().targets == ALL[:4]
    assert A.parse_lora_targets(None) == ALL[:4]
    assert A.parse_lora_targets("all-linear") == ALL
    assert A.parse_lora_targets(["down_proj", "q_proj"]) == ("q_proj", "down_proj")                # the order given is ignored
    assert A.parse_lora_targets(("up_proj",)) == ("up_proj",)
    assert A.parse_lora_targets("v_proj, gate_proj,q_proj") == ("q_proj", "v_proj", "gate_proj")
    assert A.parse_lora_targets(list(reversed(ALL))) == ALL
    assert A.parse_lora_targets("q_proj,k_proj,v_proj,o_proj") == A.parse_lora_targets(None)


@pytest.mark.parametrize("spec,word", [(["q_proj", "dense"], "dense"), ("q_proj,fc1", "fc1"), ([], "empty"), ("", "empty"), ((), "empty"),
                                       (["q_proj", "up_proj", "q_proj"], "duplicate module 'q_proj'"), ("up_proj,up_proj", "up_proj"),
                                       ("all-linear,q_proj", "all-linear"), (7, "7")])
def test_refusals_name_the_offender(spec, word):
    with pytest.raises(ValueError, match=word):
        A.parse_lora_targets(spec)


def test_default_layout_is_todays():
    """lora_layout with the default targets == the formula LlamaEngine._slices had before the keyword (q, k, v, o; A [r,d] then B [dout,r]),
    on a 2-layer grouped-query config, so that k and v are narrower."""
    c = A.LlamaCfg(256, 4, 2, 512, 256, kv_heads=2)
    r, d = 16, c.hidden
    dkv = c.kv_heads * c.head_dim
    douts = (d, dkv, dkv, d)
    per_layer = sum(r * (d + do) for do in douts)
    got_per_layer, lay = A.lora_layout(c, r, A.parse_lora_targets(None))
    assert got_per_layer == per_layer and list(lay) == list(ALL[:4])
    for i in range(c.layers):
        for j, nm in enumerate(ALL[:4]):
            base = i * per_layer + sum(r * (d + do) for do in douts[:j])
            old = ((base, base + r * d), (base + r * d, base + r * d + douts[j] * r))
            (a0, a1), (b0, b1) = lay[nm]
            assert ((i * got_per_layer + a0, i * got_per_layer + a1), (i * got_per_layer + b0, i * got_per_layer + b1)) == old


def test_layout_of_a_subset_and_of_all():
    c = A.LlamaCfg(256, 2, 2, 320, 256)
    r, d, f = 8, 256, 320
    n, lay = A.lora_layout(c, r, ("q_proj", "v_proj", "down_proj"))
    assert list(lay) == ["q_proj", "v_proj", "down_proj"] and n == r * (2 * d + 2 * d + f + d)
    assert lay["down_proj"] == ((4 * r * d, 4 * r * d + r * f), (4 * r * d + r * f, n))
    n7, lay7 = A.lora_layout(c, r, ALL)
    assert n7 == 4 * r * 2 * d + 3 * r * (d + f)
    ends = [lay7[nm][1][1] for nm in ALL]
    assert [lay7[nm][0][0] for nm in ALL] == [0] + ends[:-1] and ends[-1] == n7                   # contiguous, canonical order
    assert A.lora_shapes(c, r, "gate_proj") == ((r, d), (f, r)) and A.lora_shapes(c, r, "up_proj") == ((r, d), (f, r))
    assert A.lora_shapes(c, r, "down_proj") == ((r, f), (d, r))


def test_seed_rule_never_collides():
    """seed + 4 l + j for the attention modules, seed + 4 layers + 3 l + k for the MLP ones: distinct for every (layer, module)."""
    for layers in (1, 2, 31, 32, 255, 256):
        seeds = [R.seed_of(0, layers, l, nm) for l in range(layers) for nm in ALL]
        assert len(set(seeds)) == 7 * layers and max(seeds) == 7 * layers - 1
        assert [R.seed_of(5, layers, l, nm) for l in range(layers) for nm in ALL[:4]] == [5 + 4 * l + j for l in range(layers) for j in range(4)]


def test_key_round_trip():
    for i in (0, 31):
        for nm in ALL:
            for ab in ("lora_A", "lora_B"):
                k = A.lora_state_key(i, nm, ab)
                sec = "mlp" if nm in ALL[4:] else "self_attn"
                assert k == f"llm.base_model.model.model.layers.{i}.{sec}.{nm}.{ab}.default.weight"
                assert A.parse_lora_state_key(k) == (i, nm, ab)
    assert A.parse_lora_state_key("audio_connector.linear.weight") is None
    sd = {A.lora_state_key(1, "down_proj", "lora_A"): torch.zeros(2, 3), A.lora_state_key(0, "q_proj", "lora_B"): torch.ones(3, 2)}
    W = A.weights_from_reference_state_dict(sd)
    assert set(W["lora"]) == {"layers.1.down_proj.lora_A", "layers.0.q_proj.lora_B"}


def test_synthetic_adapters_follow_the_targets():
    """A ~ N(0, 1/r) x 0.01, B = 0 on every selected module, at its shapes; the four attention modules' draws do not depend on the rest."""
    c = A.LlamaCfg(256, 2, 2, 512, 256)
    base = A.synth_lora(c, A.LoraCfg(16, 32.0), "cpu", 3)
    full = A.synth_lora(c, A.LoraCfg(16, 32.0, ALL), "cpu", 3)
    assert all(torch.equal(base[k], full[k]) for k in base) and len(full) == 2 * 7 * 2
    assert full["layers.1.down_proj.lora_A"].shape == (16, 512) and full["layers.1.down_proj.lora_B"].shape == (256, 16)
    assert full["layers.0.gate_proj.lora_A"].shape == (16, 256) and full["layers.0.up_proj.lora_B"].shape == (512, 16)
    assert all(float(full[f"layers.{i}.{nm}.lora_B"].abs().max()) == 0 for i in range(2) for nm in ALL)
    a = full["layers.0.down_proj.lora_A"]
    assert abs(float(a.std()) - 0.01 / 16) < 0.1 * 0.01 / 16
    sub = A.synth_lora(c, A.LoraCfg(16, 32.0, ("q_proj", "up_proj")), "cpu", 3)
    assert set(sub) == {f"layers.{i}.{nm}.lora_{ab}" for i in range(2) for nm in ("q_proj", "up_proj") for ab in "AB"}


def test_reference_equals_the_oracle_on_the_default_targets():
    """With q, k, v, o adapters (and masks) the float64 restatement is the pinned oracle: llama_hidden to float64 roundoff when the oracle is
    fed float64 tensors; train_step_grads' loss, logits and gradients to the roundoff of the oracle's own arithmetic (it runs in float32)."""
    oc = Wt.tiny()
    c, lc = oc.llama, oc.lora
    sd = Wt.llama_weights(c, seed=5)
    lora = Wt.lora_weights(c, lc, seed=5, b_std=0.05)
    x, labels = R.batch(c, 2, 24)
    g = torch.Generator().manual_seed(3)
    masks = {f"layers.{l}.{nm}": (torch.rand(2, 24, c.hidden, generator=g) > 0.25).double() / 0.75 for l in range(c.layers) for nm in ALL[:4]}
    with torch.no_grad():
        want = O.llama_hidden(R.to64(sd), R.to64(lora), c, lc, x.double(), masks=masks)
        got = R.hidden(R.to64(sd), R.to64(lora), c, lc.scale, x.double(), masks)
    assert want.dtype == torch.float64 and float((got - want).abs().max()) < 1e-12 * float(want.abs().max())
    # the whole step on Wt.tiny(): the oracle's LLM inputs, its float32 loss and gradients
    W = Wt.all_weights(oc, 0, lora_b_std=0.05)
    audio, video, lab, prompt = Wt.synthetic_batch(oc, 2, 3, seed=11)
    ol, ologits, og = O.train_step_grads(W, oc, audio, video, prompt, lab)
    with torch.no_grad():
        xin, _, lab2 = O.prepare_llm_inputs(W, oc, audio, video, prompt, lab, training=True)
    loss, logits, grads, dx = R.step(W["llama"], W["lora"], c, lc.scale, xin, lab2)
    assert abs(float(loss) - float(ol)) < 1e-5 and float((logits - ologits.double()).abs().max()) < 1e-4 * float(logits.abs().max())
    assert set(grads) == set(og) and dx.shape == xin.shape and float(dx.abs().max()) > 0
    for k in og:
        assert float((grads[k] - og[k].double()).abs().max()) < 1e-4 * float(grads[k].abs().max()), k
