"""A Qwen3 LLM through the public class.  ClipWhisperModel built from `_provided_llm=Qwen3ForCausalLM(...)` (resolve_arch's `_provided_llm`
branch: model_type qwen3 -> qk_norm) and from a checkpoint directory (config.json + safetensors through `llm_path`); one training step with
train_connectors=True and generate() (greedy and num_beams=2) held to transformers' Qwen3ForCausalLM (tools/make_golden_qwen3.py's builder,
CPU fp32) run on the inputs_embeds the model itself forms; and the trainer capturing and replaying a Qwen3 step.  The LLM is case "a" of
tests/qwen3_weights.py; the encoders are the oracle's tiny Whisper and CLIP."""
import json
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import qwen3_weights as QW  # noqa: E402
from bars import rel_l2  # noqa: E402

S_OUT, NEW = 24, 8
CASE = QW.CASES["a"]


def provided(cfg_fields, sd):
    """What resolve_arch reads of a `_provided_*` module: .config and .state_dict()."""
    return SimpleNamespace(config=SimpleNamespace(**cfg_fields), state_dict=lambda: sd)


def encoders():
    from oracle import weights as Wt
    oc = Wt.tiny()
    W = Wt.all_weights(oc, 0)
    w, v = oc.whisper, oc.clip
    pw = provided(dict(d_model=w.d_model, encoder_attention_heads=w.heads, encoder_layers=w.layers, encoder_ffn_dim=w.ffn, num_mel_bins=w.n_mels,
                       max_source_positions=w.n_ctx), W["whisper"])
    pc = provided(dict(hidden_size=v.hidden, num_attention_heads=v.heads, num_hidden_layers=v.layers, intermediate_size=v.mlp, image_size=v.image,
                       patch_size=v.patch, layer_norm_eps=v.eps), W["clip"])
    return oc, pw, pc


def make_model(precision="fp32", dropout=0.0, **kw):
    from avllm.model import ClipWhisperModel
    _, pw, pc = encoders()
    _, lora = QW.weights(CASE)
    return ClipWhisperModel(kw.pop("llm_path", "qwen3-tiny"), "whisper-tiny", "clip-tiny", device="cuda:0", use_lora=True, lora_r=QW.RANK, lora_alpha=QW.ALPHA,
                            lora_dropout=dropout, max_seq_len=256, _provided_whisper=pw, _provided_clip=pc, precision=precision, weights={"lora": lora},
                            train_connectors=True, **kw)


def batch(dev):
    from oracle import weights as Wt
    audio, video, _, _ = Wt.synthetic_batch(encoders()[0], 2, 5, seed=7)
    g = torch.Generator().manual_seed(11)
    prompt = torch.randint(3, CASE.vocab, (2, 6), generator=g)
    labels = torch.randint(3, CASE.vocab, (2, S_OUT), generator=g)
    labels[:, :4] = -100
    return audio.to(dev), video.to(dev), prompt.to(dev), labels


@pytest.fixture(scope="module")
def mk():
    pytest.importorskip("transformers")
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import make_golden_qwen3
    return make_golden_qwen3


@pytest.fixture(scope="module")
def built(dev, mk):
    sd, lora = QW.weights(CASE)
    m = make_model(_provided_llm=mk.build_hf(CASE, sd, None))
    audio, video, prompt, labels = batch(dev)
    return m, mk.build_hf(CASE, sd, lora), (audio, video, prompt), labels


def test_provided_qwen3_resolves_to_qk_norm(built):
    m = built[0]
    c = m.cfg.llama
    assert (c.qk_norm, c.qkv_bias, c.o_bias, c.theta, c.eps, c.kv_heads, c.hidden, c.heads) == (True, False, False, 1e6, 1e-6, 2, 512, 4)
    assert all(ly.q_norm_w and ly.k_norm_w and not ly.bqkv for ly in m.llm_engine.layers)


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
    print(f"ClipWhisperModel(Qwen3) fp32: max |dlogits| {dl:.2e}, |dloss| {abs(float(out['loss'].detach()) - float(ref.loss.detach())):.2e}")
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


def test_beam_search_matches_transformers(dev, built):
    """num_beams=2 through the B * 2-row token steps and the KV reorder (the cache holds post-norm k rows, which is what moves): the best
    hypothesis and its score are transformers' where its own two hypotheses are further apart than the fp32 bar allows the scores to move."""
    m, hf, (audio, video, prompt), _ = built
    m.eval()
    ids, scores = m.generate(audio=audio, video=video, prompt=prompt, max_new_tokens=NEW, num_beams=2, return_sequence_scores=True)
    ids, scores = ids.cpu(), scores.cpu()
    assert ids.shape[0] == 2 and 1 <= ids.shape[1] <= NEW and torch.isfinite(scores).all()
    x = m._llm_inputs(audio, video, prompt).float().cpu()
    with torch.no_grad():
        gen = hf.generate(inputs_embeds=x, attention_mask=torch.ones(x.shape[:2], dtype=torch.long), max_new_tokens=NEW, do_sample=False, num_beams=2,
                          num_return_sequences=2, eos_token_id=m.eos_token_id, pad_token_id=m.tokenizer.pad_token_id, output_scores=True,
                          return_dict_in_generate=True)
    seqs, ss = gen.sequences.view(2, 2, -1), gen.sequences_scores.view(2, 2)
    compared = 0
    for b in range(2):
        gap = float(ss[b, 0] - ss[b, 1])
        print(f"beam row {b}: transformers' best {float(ss[b, 0]):.5f} over its runner-up by {gap:.5f}; generate() {float(scores[b]):.5f}")
        if gap >= 2.0 * Bar.F32_LOGITS_ABS:
            n = min(ids.shape[1], seqs.shape[2])
            assert torch.equal(ids[b, :n], seqs[b, 0, :n]), (b, ids[b].tolist(), seqs[b, 0].tolist())
            assert abs(float(scores[b]) - float(ss[b, 0])) < Bar.F32_LOGITS_ABS
            compared += 1
    assert compared >= 1


def test_checkpoint_directory_gives_the_same_logits(dev, built, tmp_path):
    """config.json (model_type qwen3) + model.safetensors through llm_path: the same model as the `_provided_llm` one, bit for bit."""
    from safetensors.torch import save_file
    m, _, (audio, video, prompt), labels = built
    sd, _ = QW.weights(CASE)
    (tmp_path / "config.json").write_text(json.dumps(QW.hf_config_dict(CASE)))
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "model.safetensors"))
    m2 = make_model(llm_path=str(tmp_path))
    assert m2.cfg.llama == m.cfg.llama and m2.cfg.llama.qk_norm
    m.train()
    m2.train()
    a = m(audio=audio, video=video, prompt=prompt, labels=labels.to(dev))["logits"]
    b = m2(audio=audio, video=video, prompt=prompt, labels=labels.to(dev))["logits"]
    assert torch.equal(a, b)
    m2.eval()
    m.eval()
    assert torch.equal(m2.generate(audio=audio, video=video, prompt=prompt, max_new_tokens=4), m.generate(audio=audio, video=video, prompt=prompt, max_new_tokens=4))


def test_trainer_moves_connectors_and_graph_replay_equals_eager(dev, mk):
    """Three trainer steps with train_connectors=True, LoRA dropout and clipping, eager and captured (step 2 captured, step 3 replayed): the
    connector tensors and the adapters move, and the replayed run equals the eager one by the rule of
    test_pin_bf16_gpu.py::test_graph_replayed_step_matches_eager_step (bf16: losses within 2e-3, parameters within 2e-2 relative L2)."""
    from avllm.trainer import ClipWhisperTrainer
    sd, _ = QW.weights(CASE)
    audio, video, prompt, labels = batch(dev)
    runs = {}
    for graph in (False, True):
        m = make_model("bf16", dropout=0.05, _provided_llm=mk.build_hf(CASE, sd, None)).train()
        conn0, lora0 = m.conn_p.clone(), m.llm_engine.lora_p.clone()
        tr = ClipWhisperTrainer(m, learning_rate=1e-3, total_steps=10, max_epochs=1, grad_clip=0.5, use_graph=graph)
        losses = [float(tr.train_step(audio, video, labels.to(dev), prompt)) for _ in range(3)]
        assert all(l == l and abs(l) < 1e3 for l in losses)
        assert float((m.conn_p - conn0).abs().max()) > 0 and float((m.llm_engine.lora_p - lora0).abs().max()) > 0
        if graph:
            assert any(isinstance(v, dict) for v in tr._graphs.values())
        runs[graph] = (losses, m.conn_p.clone().cpu(), m.llm_engine.lora_p.clone().cpu(), conn0.cpu(), lora0.cpu())
    (l0, c0, p0, ci, pi), (l1, c1, p1, _, _) = runs[False], runs[True]
    assert max(abs(a - b) for a, b in zip(l0, l1)) < 2e-3, (l0, l1)
    assert rel_l2(p1, p0) < 2e-2 and rel_l2(c1, c0) < 2e-2
    assert rel_l2(p1 - pi, p0 - pi) < 0.5 and rel_l2(c1 - ci, c0 - ci) < 0.5          # the UPDATES agree too, not just the parameters they are small against


def test_sampled_and_processed_generate_run_on_the_same_steps(dev, built):
    """What does not touch the projections needs no change but must run: top_k = 1 sampling is the greedy sequence, and the logits processors
    edit the same logits (a banned repeat never appears)."""
    m, _, (audio, video, prompt), _ = built
    m.eval()
    greedy = m.generate(audio=audio, video=video, prompt=prompt, max_new_tokens=NEW)
    assert torch.equal(m.generate(audio=audio, video=video, prompt=prompt, max_new_tokens=NEW, do_sample=True, top_k=1, seed=3), greedy)
    ids = m.generate(audio=audio, video=video, prompt=prompt, max_new_tokens=NEW, no_repeat_ngram_size=1, repetition_penalty=1.3).cpu()
    for row in ids.tolist():
        toks = [t for t in row if t != m.tokenizer.pad_token_id]
        assert len(set(toks)) == len(toks), row


@pytest.mark.parametrize("form", ["fp8", "fp4"])
def test_weight_only_generate_streams_the_codes(dev, mk, form):
    sd, _ = QW.weights(CASE)
    audio, video, prompt, _ = batch(dev)
    m = make_model("bf16", _provided_llm=mk.build_hf(CASE, sd, None), decode_weights=form).eval()
    eng = m.llm_engine
    assert eng.decode_is_fused(2) and eng.decode_streams_fp8(2) == (form == "fp8") and eng.decode_streams_fp4(2) == (form == "fp4")
    ids = m.generate(audio=audio, video=video, prompt=prompt, max_new_tokens=NEW).cpu()
    assert ids.shape[0] == 2 and 1 <= ids.shape[1] <= NEW and bool(((ids >= 0) & (ids < CASE.vocab)).all())
