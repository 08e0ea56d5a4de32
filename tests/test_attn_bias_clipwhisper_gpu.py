"""A Qwen2 LLM through the public class: ClipWhisperModel built from `_provided_*` modules (the reference's constructor arguments), so the
architecture comes out of resolve_arch's `_provided_llm` branch (model_type qwen2 -> qkv_bias) and the weights out of the module's state dict.
Training forward / backward with train_connectors=True and generate() are held to transformers' Qwen2ForCausalLM (tools/make_golden_qwen2.py's
builder, CPU fp32) run on the inputs_embeds the model itself forms.  The LLM is case "q" of tests/attn_bias_weights.py; the encoders are the
oracle's tiny Whisper and CLIP."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_bias_weights as AW  # noqa: E402
import bars as Bar  # noqa: E402

S_OUT, NEW = 24, 8


def provided(cfg_fields, sd):
    """What resolve_arch reads of a `_provided_*` module: .config and .state_dict()."""
    return SimpleNamespace(config=SimpleNamespace(**cfg_fields), state_dict=lambda: sd)


@pytest.fixture(scope="module")
def built(dev):
    pytest.importorskip("transformers")
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import make_golden_qwen2 as mk
    from avllm.model import ClipWhisperModel
    from oracle import weights as Wt
    oc = Wt.tiny()
    W = Wt.all_weights(oc, 0)
    w, v = oc.whisper, oc.clip
    pw = provided(dict(d_model=w.d_model, encoder_attention_heads=w.heads, encoder_layers=w.layers, encoder_ffn_dim=w.ffn, num_mel_bins=w.n_mels,
                       max_source_positions=w.n_ctx), W["whisper"])
    pc = provided(dict(hidden_size=v.hidden, num_attention_heads=v.heads, num_hidden_layers=v.layers, intermediate_size=v.mlp, image_size=v.image,
                       patch_size=v.patch, layer_norm_eps=v.eps), W["clip"])
    c = AW.CASES["q"]
    sd, lora = AW.weights(c)
    m = ClipWhisperModel("qwen2-tiny", "whisper-tiny", "clip-tiny", device="cuda:0", use_lora=True, lora_r=AW.RANK, lora_alpha=AW.ALPHA, lora_dropout=0.0,
                         max_seq_len=256, _provided_llm=mk.build_hf(c, sd, None), _provided_whisper=pw, _provided_clip=pc, precision="fp32",
                         weights={"lora": lora}, train_connectors=True)
    audio, video, _, _ = Wt.synthetic_batch(oc, 2, 5, seed=7)
    g = torch.Generator().manual_seed(11)
    prompt = torch.randint(3, c.vocab, (2, 6), generator=g)
    labels = torch.randint(3, c.vocab, (2, S_OUT), generator=g)
    labels[:, :4] = -100
    return m, mk.build_hf(c, sd, lora), (audio.to(dev), video.to(dev), prompt.to(dev)), labels


def test_provided_qwen2_resolves_to_qkv_bias(built):
    m = built[0]
    c = m.cfg.llama
    assert (c.qkv_bias, c.o_bias, c.theta, c.eps, c.kv_heads, c.hidden, c.heads) == (True, False, 1e6, 1e-6, 2, 896, 14)
    assert all(ly.bqkv and not ly.bo for ly in m.llm_engine.layers)


def test_training_step_matches_transformers(dev, built):
    m, hf, (audio, video, prompt), labels = built
    m.train()
    out = m(audio=audio, video=video, prompt=prompt, labels=labels.to(dev))
    m.lora_param.grad = None
    out["loss"].backward()
    torch.cuda.synchronize()
    dx = m._dx_embeds_buffer().float().cpu().clone()
    x = m._llm_inputs(audio, video, prompt, S_out=S_OUT).float().cpu()
    xg = x.clone().requires_grad_(True)
    ref = hf(inputs_embeds=xg, labels=labels)
    ref.loss.backward()
    dl = float((out["logits"].float().cpu() - ref.logits.detach()).abs().max())
    print(f"ClipWhisperModel(Qwen2) fp32: max |dlogits| {dl:.2e}, |dloss| {abs(float(out['loss'].detach()) - float(ref.loss.detach())):.2e}")
    assert dl < Bar.F32_LOGITS_ABS
    assert abs(float(out["loss"].detach()) - float(ref.loss.detach())) < Bar.F32_LOSS_ABS
    gv = m.llm_engine.lora_views(m.lora_param.grad)
    for i, layer in enumerate(hf.model.layers):
        for nm in ("q_proj", "k_proj", "v_proj", "o_proj"):
            mod = getattr(layer.self_attn, nm)
            for key, g in ((f"layers.{i}.{nm}.lora_A", mod.lora_A.grad), (f"layers.{i}.{nm}.lora_B", mod.lora_B.grad)):
                assert float((gv[key].cpu() - g).abs().max()) <= Bar.F32_GRAD_REL_MAX * float(g.abs().max()), key
            mod.lora_A.grad = mod.lora_B.grad = None
    assert float((dx - xg.grad).abs().max()) <= Bar.F32_GRAD_REL_MAX * float(xg.grad.abs().max())
    for conn in (m.audio_connector, m.video_connector):
        for p in conn.parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0


def test_generate_matches_transformers(dev, built):
    m, hf, (audio, video, prompt), _ = built
    m.eval()
    ids = m.generate(audio=audio, video=video, prompt=prompt, max_new_tokens=NEW).cpu()
    x = m._llm_inputs(audio, video, prompt).float().cpu()
    with torch.no_grad():
        gen = hf.generate(inputs_embeds=x, attention_mask=torch.ones(x.shape[:2], dtype=torch.long), max_new_tokens=NEW, do_sample=False,
                          output_scores=True, return_dict_in_generate=True, pad_token_id=0)
    top = torch.stack(gen.scores, 1).topk(2, -1).values
    margin = top[..., 0] - top[..., 1]
    compared = 0
    for b in range(ids.shape[0]):
        for t in range(min(ids.shape[1], NEW)):
            if int(gen.sequences[b, t]) == m.eos_token_id:
                break                                            # transformers runs without an EOS here; past it the two loops differ by design
            same = int(ids[b, t]) == int(gen.sequences[b, t])
            if float(margin[b, t]) >= 2.0 * Bar.F32_LOGITS_ABS:
                assert same, (b, t, ids[b].tolist(), gen.sequences[b].tolist(), margin[b].tolist())
                compared += 1
            elif not same:
                break
    assert compared >= 8, (compared, margin.tolist())
