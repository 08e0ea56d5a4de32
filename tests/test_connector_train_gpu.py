"""train_connectors=True on the GPU (tiny golden model): d(inputs_embeds) and the four connector gradients against the CPU-made expectation
(tests/connector_expect.py: autograd through the existing oracle functions, itself pinned to the reference in test_connector_grads_cpu.py)
and the reference's own values (tests/golden/g11_connector_grads.npz, case "b"); the trainer step with connectors against the oracle's loop;
graph replay == eager; the non-finite guard; checkpoints; loss.backward(); the flag off; the refusals.

Label widths: 24 columns take the pool branch (32 + 512 rows -> 24), 64 columns with max_seq_len = 16 the interpolate branch (32 + 16 -> 64;
there every label position is scored, so that positions behind the stretched prompt rows -- the only ones that see fused rows -- count).
fp32 bar: bars.F32_GRAD_REL_MAX (what LoRA gradients are held to in fp32); bf16 bar: bars.BF16_GRAD_REL_L2 on the whole connector gradient.
lora_dropout 0.05 hands the kernels' own masks to the oracle (as tests/test_pin_bf16_gpu.py does): fp32 runs layer 0's per-adapter masked
GEMMs, bf16 the fused av_lora_dx_masked branch."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import connector_expect as CE  # noqa: E402
from oracle import avsr_oracle as O  # noqa: E402
from oracle import weights as Wt  # noqa: E402

GEO = {"pool": (512, 24), "interp": (16, 64)}          # name -> (max_seq_len, label columns)


def make_model(oc, W, precision, max_seq_len=512, dropout=0.0, train_connectors=True, **kw):
    from avllm.arch import ClipCfg, LlamaCfg, LoraCfg, ModelCfg, WhisperCfg
    from avllm.model import ClipWhisperModel
    cfg = ModelCfg(WhisperCfg(**vars(oc.whisper)), ClipCfg(**vars(oc.clip)), LlamaCfg(**vars(oc.llama)), LoraCfg(oc.lora.r, oc.lora.alpha))
    return ClipWhisperModel(device="cuda:0", lora_r=oc.lora.r, lora_alpha=oc.lora.alpha, lora_dropout=dropout, max_seq_len=max_seq_len, config=cfg,
                            weights=W, precision=precision, train_connectors=train_connectors, **kw).train()


@pytest.fixture(scope="module")
def tiny(golden_dir):
    z = np.load(os.path.join(golden_dir, "g11_connector_grads.npz"))
    oc = Wt.tiny()
    W = Wt.all_weights(oc, int(z["seed"]), lora_b_std=0.05)
    audio, video, labels, _ = Wt.synthetic_batch(oc, 2, int(z["frames"]), seed=int(z["batch_seed"]))
    return z, oc, W, audio, video, labels, torch.from_numpy(z["prompt"])


def batch_for(tiny, geo):
    z, oc, W, audio, video, labels, prompt = tiny
    msl, cols = GEO[geo]
    oc2 = copy.deepcopy(oc)
    oc2.max_seq_len = msl
    lab = labels[:, :cols].contiguous()
    if geo == "interp":
        # the synthetic transcripts are 8..40 tokens long; stretched from 48 to 64 rows, the fused rows sit behind label position 42, which under
        # causal attention no scored token of such a transcript sees (the connectors' gradient would be exactly zero): score every position
        lab[:, 1:] = torch.randint(3, oc.llama.vocab, (lab.shape[0], cols - 1), generator=torch.Generator().manual_seed(5))
    return oc2, W, audio, video, lab, prompt


_EXPECT = {}


def expectation(tiny, geo, masks=None, key=None):
    """The oracle's step, computed once per (geometry, mask set) and shared."""
    k = (geo, key)
    if k not in _EXPECT:
        oc2, W, audio, video, lab, prompt = batch_for(tiny, geo)
        _EXPECT[k] = CE.connector_step(W, oc2, audio, video, prompt, lab, masks=masks)
    return _EXPECT[k]


def masks_of(m, B, S, p, dev):
    from avllm import ops
    eng = m.llm_engine
    ones = torch.ones(B * S, eng.cfg.hidden, device=dev, dtype=torch.float32)
    return {f"layers.{l}.{nm}": ops.dropout(ones, eng.desc.dropout_seed + 4 * l + j, p).cpu().view(B, S, -1)
            for l in range(eng.cfg.layers) for j, nm in enumerate(("q_proj", "k_proj", "v_proj", "o_proj"))}


def conn_grads(m):
    return {k: p.grad.detach().float().cpu() for k, p in m.named_parameters() if "connector" in k}


@pytest.mark.parametrize("p", [0.0, 0.05])
@pytest.mark.parametrize("geo", ["pool", "interp"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_dx_embeds_and_connector_grads_vs_oracle(dev, tiny, precision, geo, p):
    oc2, W, audio, video, lab, prompt = batch_for(tiny, geo)
    m = make_model(oc2, W, precision, max_seq_len=GEO[geo][0], dropout=p)
    out = m(audio=audio.to(dev), video=video.to(dev), prompt=prompt.to(dev), labels=lab.to(dev))
    out["loss"].backward()
    B, S = lab.shape
    masks = masks_of(m, B, S, p, dev) if p else None
    loss, dx, grads, _ = expectation(tiny, geo, masks, key=(p, m.llm_engine.desc.dropout_seed if p else 0))
    got_dx = m._dx_embeds_buffer().float().cpu()
    got = conn_grads(m)
    assert set(got) == set(CE.CONNECTOR_KEYS)
    assert all(float(grads[k].abs().max()) > 1e-4 for k in CE.CONNECTOR_KEYS)          # every tensor has a gradient to be wrong about
    if precision == "fp32":
        assert abs(float(out["loss"].detach()) - float(loss)) < Bar.F32_LOSS_ABS
        for name, a, b in [("dx_embeds", got_dx, dx)] + [(k, got[k], grads[k]) for k in CE.CONNECTOR_KEYS]:
            d = float((a - b).abs().max())
            print(f"{precision} {geo} p={p} {name}: max |diff| {d:.3e}, max |ref| {float(b.abs().max()):.3e}")
            assert d <= Bar.F32_GRAD_REL_MAX * float(b.abs().max()), (name, d, float(b.abs().max()))
    else:
        assert abs(float(out["loss"].detach()) - float(loss)) < Bar.BF16_LOSS_ABS
        allg = torch.cat([got[k].flatten() for k in CE.CONNECTOR_KEYS])
        allo = torch.cat([grads[k].flatten() for k in CE.CONNECTOR_KEYS])
        print(f"{precision} {geo} p={p}: connector gradient rel L2 {Bar.rel_l2(allg, allo):.3e}, dx_embeds rel L2 {Bar.rel_l2(got_dx, dx):.3e}")
        assert Bar.rel_l2(allg, allo) < Bar.BF16_GRAD_REL_L2
        assert Bar.rel_l2(got_dx, dx) < Bar.BF16_GRAD_REL_L2
    if precision == "fp32" and geo == "pool" and p == 0.0:          # the reference's own numbers for this very case
        z = tiny[0]
        for k in CE.CONNECTOR_KEYS:
            ref = torch.from_numpy(z["b.grad." + k])
            assert float((got[k] - ref).abs().max()) <= Bar.F32_GRAD_REL_MAX * float(ref.abs().max()), k


def test_grouped_query_connector_grads_fp32(dev):
    """The g7 geometry: 4 query heads over 2 key / value heads (layer 0's dqkv . Wqkv product is narrower than 3 d)."""
    oc = Wt.tiny()
    oc.llama = Wt.LlamaCfg(hidden=256, heads=4, layers=2, ffn=512, vocab=256, kv_heads=2)
    W = Wt.all_weights(oc, 3, lora_b_std=0.05)
    audio, video, labels, _ = Wt.synthetic_batch(oc, 2, 5, seed=77)
    prompt = torch.randint(3, oc.llama.vocab, (2, 20), generator=torch.Generator().manual_seed(5))
    lab = labels[:, :24].contiguous()
    m = make_model(oc, W, "fp32")
    m(audio=audio.to(dev), video=video.to(dev), prompt=prompt.to(dev), labels=lab.to(dev))["loss"].backward()
    _, dx, grads, _ = CE.connector_step(W, oc, audio, video, prompt, lab)
    got = conn_grads(m)
    for name, a, b in [("dx_embeds", m._dx_embeds_buffer().float().cpu(), dx)] + [(k, got[k], grads[k]) for k in CE.CONNECTOR_KEYS]:
        assert float(b.abs().max()) > 1e-4
        assert float((a - b).abs().max()) <= Bar.F32_GRAD_REL_MAX * float(b.abs().max()), name


@pytest.mark.parametrize("precision,p", [("fp32", 0.0), ("bf16", 0.05)])
def test_lora_grads_unchanged_by_dx_embeds(dev, tiny, precision, p):
    """The same step with and without dx_embeds: the LoRA gradient is the same bits (layer 0 only ADDS launches after its adapters' gradients)."""
    oc2, W, audio, video, lab, prompt = batch_for(tiny, "pool")
    m = make_model(oc2, W, precision, dropout=p)
    eng = m.llm_engine
    res = []
    for with_dx in (True, False):
        x = m._llm_inputs(audio.to(dev), video.to(dev), prompt.to(dev), S_out=lab.shape[1], keep=True)
        eng.fwd_loss(x, m._prep_labels(lab.to(dev)), dropout=p, seed=1234)
        eng.lora_g.zero_()
        eng.bwd(dx_embeds=m._dx_embeds_buffer() if with_dx else None)
        res.append(eng.lora_g.clone())
    assert float(res[0].abs().max()) > 0 and torch.equal(res[0], res[1])


def test_trainer_three_steps_vs_oracle(dev, tiny):
    """AdamW with the two decay groups (connector weights and LoRA decayed, connector biases not), ONE clip at 0.5 over connector and LoRA
    gradients together, cosine schedule: the bars of tests/test_model_gpu.py::test_trainer_steps_vs_oracle."""
    from avllm.trainer import ClipWhisperTrainer
    oc2, W, audio, video, lab, prompt = batch_for(tiny, "pool")
    m = make_model(oc2, W, "fp32")
    tr = ClipWhisperTrainer(m, learning_rate=1e-3, weight_decay=0.01, grad_clip=0.5, total_steps=10, max_epochs=1)
    Wo = dict(W)
    Wo["lora"] = {k: v.clone() for k, v in W["lora"].items()}
    for n in ("audio_connector", "video_connector"):
        Wo[n] = {k: v.clone() for k, v in W[n].items()}
    par = {"lora." + k: v for k, v in Wo["lora"].items()}
    par.update({f"{n}.{k}": v for n in ("audio_connector", "video_connector") for k, v in Wo[n].items()})
    keys = sorted(par)
    mo, vo = {k: torch.zeros_like(par[k]) for k in keys}, {k: torch.zeros_like(par[k]) for k in keys}
    for s in range(3):
        loss = tr.train_step(audio.to(dev), video.to(dev), lab.to(dev), prompt.to(dev))
        ol, _, cg, lg = CE.connector_step(Wo, oc2, audio, video, prompt, lab)
        assert abs(float(loss) - float(ol)) < 2e-4, (s, float(loss), float(ol))
        g = {"lora." + k: v for k, v in lg.items()}
        g.update(cg)
        gl = [g[k] for k in keys]
        O.clip_grad_norm_(gl, 0.5)
        for k, gk in zip(keys, gl):
            O.adamw_step(par[k], gk, mo[k], vo[k], s + 1, O.cosine_lr(1e-3, s, 10), wd=0.0 if k.endswith("bias") else 0.01)
    have = {"lora." + k: v.cpu() for k, v in m.llm_engine.lora_views().items()}
    have.update({k: p.detach().cpu() for k, p in m.named_parameters() if "connector" in k})
    init = {"lora." + k: v for k, v in W["lora"].items()}
    init.update({f"{n}.{k}": v for n in ("audio_connector", "video_connector") for k, v in W[n].items()})
    for group in (lambda k: k.startswith("lora."), lambda k: "connector" in k):
        num = den = 0.0
        for k in filter(group, keys):
            upd_ref = par[k] - init[k]
            num += float(((have[k] - init[k]) - upd_ref).pow(2).sum()); den += float(upd_ref.pow(2).sum())
        assert den > 0 and (num / den) ** 0.5 < 2e-2, (num / den) ** 0.5
    for k in CE.CONNECTOR_KEYS:
        assert float((have[k] - init[k]).abs().max()) > 1e-4, k          # every connector tensor moved


def _run(tiny, dev, graph, steps, precision="fp32", p=0.05, ckpt=None, tmp=None):
    from avllm.trainer import ClipWhisperTrainer
    oc2, W, audio, video, lab, prompt = batch_for(tiny, "pool")
    m = make_model(oc2, W, precision, dropout=p)
    tr = ClipWhisperTrainer(m, learning_rate=1e-3, total_steps=10, max_epochs=1, grad_clip=0.5, use_graph=graph, output_dir=str(tmp) if tmp else "outputs/x")
    if ckpt:
        tr.load_checkpoint(ckpt)
    losses = [float(tr.train_step(audio.to(dev), video.to(dev), lab.to(dev), prompt.to(dev))) for _ in range(steps)]
    return m, tr, losses


def same_loss(a, b, rows=48):
    """Two runs of one step report the same loss up to the order in which avllm_ce_fwd's float atomics add the rows' terms onto loss_sum
    (bars.atomic_sum_term; the count is exact).  Nothing in the backward pass or the optimizer reads loss_sum beyond its finiteness, so
    parameters, gradients and moments are compared bit for bit."""
    return abs(a - b) <= Bar.atomic_sum_term(rows, max(abs(a), abs(b)))


def test_graph_replay_equals_eager_with_connectors(dev, tiny):
    m0, t0, l0 = _run(tiny, dev, False, 3)
    m1, t1, l1 = _run(tiny, dev, True, 3)
    assert any(isinstance(v, dict) for v in t1._graphs.values())          # step 2 captured, step 3 replayed
    assert all(same_loss(a, b) for a, b in zip(l0, l1)), (l0, l1)
    assert torch.equal(m0.conn_p, m1.conn_p) and torch.equal(m0.llm_engine.lora_p, m1.llm_engine.lora_p)
    assert torch.equal(t0.cm, t1.cm) and torch.equal(t0.cv, t1.cv)
    assert float((m0.conn_p - make_model(*batch_for(tiny, "pool")[:2], "fp32").conn_p).abs().max()) > 0


def test_checkpoint_round_trip_with_connectors(dev, tiny, tmp_path):
    m_full, _, l_full = _run(tiny, dev, False, 3)
    m_a, tr_a, _ = _run(tiny, dev, False, 2, tmp=tmp_path)
    tr_a._save_checkpoint(0, "ck.pt")
    ck = torch.load(os.path.join(str(tmp_path), "ck.pt"), weights_only=True)
    st = ck["optimizer_state_dict"]
    n_lora = len(tr_a._lora_keys())
    assert len(st["state"]) == 4 + n_lora and tuple(st["state"][0]["exp_avg"].shape) == tuple(m_a.audio_connector.linear.weight.shape)
    assert st["param_groups"][1]["weight_decay"] == 0.0 and st["param_groups"][1]["params"] == [1, 3]
    assert ck["model_state_dict"]["audio_connector.linear.weight"].dtype == torch.float32
    m_b, tr_b, l_b = _run(tiny, dev, False, 1, ckpt=os.path.join(str(tmp_path), "ck.pt"))
    assert same_loss(l_b[0], l_full[2]), (l_b, l_full)
    assert torch.equal(m_b.conn_p, m_full.conn_p) and torch.equal(m_b.llm_engine.lora_p, m_full.llm_engine.lora_p)


def test_nonfinite_batch_touches_nothing_and_counts_once(dev, tiny):
    """good, BAD, good == good, good: no connector or LoRA tensor changes on the bad batch, skipped_steps == 1, and the following step's lr and
    bias corrections are those of a run that never saw it (tests/test_trainer_robust_gpu.py)."""
    from avllm.trainer import ClipWhisperTrainer
    oc2, W, audio, video, lab, prompt = batch_for(tiny, "pool")
    bad_audio = audio.clone()
    bad_audio[0, 0, 0] = float("nan")
    for graph in (False, True):
        runs = []
        for seq in ((audio, bad_audio, bad_audio, audio, audio), (audio, audio, audio)):
            m = make_model(oc2, W, "fp32")
            tr = ClipWhisperTrainer(m, learning_rate=1e-3, total_steps=10, max_epochs=1, warmup_steps=2, grad_clip=0.5, use_graph=graph)
            for a in seq:
                before = (m.conn_p.clone(), m.llm_engine.lora_p.clone(), tr.cm.clone(), tr.m.clone())
                loss = tr.train_step(a.to(dev), video.to(dev), lab.to(dev), prompt.to(dev))
                if a is bad_audio:
                    assert not bool(torch.isfinite(loss))
                    after = (m.conn_p, m.llm_engine.lora_p, tr.cm, tr.m)
                    assert all(torch.equal(x, y) for x, y in zip(before, after))
            runs.append((m, tr))
        (m, tr), (mr, trr) = runs
        assert tr.skipped_steps == 2 and trr.skipped_steps == 0 and tr._sync_step() == 3 == trr._sync_step()
        assert float(tr.state.cpu().numpy().view(np.float32)[5]) == 2.0                          # state.skipped: once per bad step
        assert torch.equal(tr.state.cpu()[8:20], trr.state.cpu()[8:20])                          # lr, bc1, bc2_sqrt of the last step
        rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
        assert rel(m.conn_p, mr.conn_p) < 1e-5 and rel(m.llm_engine.lora_p, mr.llm_engine.lora_p) < 1e-5


def test_loss_backward_fills_connector_grads_like_the_trainer_path(dev, tiny):
    from avllm.trainer import ClipWhisperTrainer
    oc2, W, audio, video, lab, prompt = batch_for(tiny, "pool")
    m = make_model(oc2, W, "fp32")
    m(audio=audio.to(dev), video=video.to(dev), prompt=prompt.to(dev), labels=lab.to(dev))["loss"].backward()
    user = torch.cat([p.grad.flatten() for k, p in m.named_parameters() if "connector" in k])
    assert [k for k, _ in m.named_parameters()][:4] == list(CE.CONNECTOR_KEYS)
    assert all(p.requires_grad and p.dtype == torch.float32 for k, p in m.named_parameters() if "connector" in k)
    tr = ClipWhisperTrainer(m, use_graph=False)
    tr._part_fwd(audio.to(dev), video.to(dev), lab.to(dev), prompt.to(dev))
    tr._part_bwd(0)
    assert float(user.abs().max()) > 0 and torch.equal(user, m.conn_g)


def test_flag_off_connectors_stay_frozen_and_bit_identical(dev, tiny):
    from avllm.trainer import ClipWhisperTrainer
    oc2, W, audio, video, lab, prompt = batch_for(tiny, "pool")
    m = make_model(oc2, W, "bf16", train_connectors=False)
    assert not m.train_connectors and not hasattr(m, "conn_p")
    ps = [p for k, p in m.named_parameters() if "connector" in k]
    assert len(ps) == 4 and not any(p.requires_grad for p in ps) and all(p.dtype == torch.bfloat16 for p in ps)
    before = [p.detach().clone() for p in ps]
    tr = ClipWhisperTrainer(m, learning_rate=1e-3, total_steps=10, max_epochs=1)
    for _ in range(2):
        tr.train_step(audio.to(dev), video.to(dev), lab.to(dev), prompt.to(dev))
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, ps)) and all(p.grad is None for p in ps)


def test_refusals(dev, tiny):
    _, oc, W, *_ = tiny
    for kw, exc in (({"connector_type": "deep"}, NotImplementedError), ({"connector_type": "conv"}, NotImplementedError),
                    ({"precision": "fp8"}, NotImplementedError), ({"use_lora": False}, ValueError)):
        prec = kw.pop("precision", "bf16")
        with pytest.raises(exc, match="train_connectors"):
            make_model(oc, W, prec, **kw)
    with pytest.raises(NotImplementedError, match="freeze_encoders"):
        make_model(oc, W, "fp32", freeze_encoders=False)


def test_state_dict_and_save_pretrained_carry_the_masters(dev, tiny, tmp_path):
    _, oc, W, *_ = tiny
    m = make_model(oc, W, "bf16")
    sd = m.state_dict()
    off = make_model(oc, W, "bf16", train_connectors=False).state_dict()
    assert set(sd) == set(off)                                            # same keys as with the flag off
    assert sd["audio_connector.linear.weight"].dtype == torch.float32
    assert torch.equal(sd["video_connector.linear.weight"].cpu(), W["video_connector"]["linear.weight"])
    m.conn_p.mul_(0.5)
    m.load_state_dict(sd)
    assert torch.equal(m.audio_connector.linear.weight.detach().cpu(), W["audio_connector"]["linear.weight"])
    assert m.audio_connector.linear.weight.data_ptr() == m.conn_p.data_ptr()              # still views of the flat buffer
    assert torch.equal(m.audio_connector.operands()[0].cpu(), W["audio_connector"]["linear.weight"].to(torch.bfloat16))      # image refreshed
    m.save_pretrained(str(tmp_path))
    assert torch.load(os.path.join(str(tmp_path), "audio_connector.pt"), weights_only=True)["linear.weight"].dtype == torch.float32
