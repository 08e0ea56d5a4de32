"""Per-clip modality through the model on the GPU (tiny model, three clips): forward() / encode() / generate() with modality_mask, the draw in
train() mode against its restatement (tests/refs64_modality.py), the connector gradients of a clip that lost its video, the refusals.
fp32 throughout: rows of a batch do not interact, so per-clip statements are bit-for-bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64_modality as RM  # noqa: E402
from oracle import weights as Wt  # noqa: E402
from test_connector_train_gpu import conn_grads, make_model  # noqa: E402

B, MIXED = 3, [0, 1, 2]


@pytest.fixture(scope="module")
def setup():
    oc = Wt.tiny()
    W = Wt.all_weights(oc, 7, lora_b_std=0.05)
    audio, video, labels, _ = Wt.synthetic_batch(oc, B, 5, seed=11)
    prompt = torch.randint(3, oc.llama.vocab, (B, 20), generator=torch.Generator().manual_seed(5))
    return oc, W, audio, video, labels[:, :24].contiguous(), prompt


@pytest.fixture(scope="module")
def model(dev, setup):
    oc, W, *_ = setup
    return make_model(oc, W, "fp32", max_seq_len=64, train_connectors=False).eval()


def other(t, rows, seed):
    """t with the given clips replaced by other random data."""
    out = t.clone()
    out[rows] = torch.randn(out[rows].shape, generator=torch.Generator().manual_seed(seed))
    return out


def test_forward_mask_all_zero_is_the_default_call(dev, setup, model):
    _, _, audio, video, _, prompt = setup
    a, v, p = audio.to(dev), video.to(dev), prompt.to(dev)
    base = model(audio=a, video=v, prompt=p)["logits"]
    assert model.last_modality_modes is None
    for mask in ([0] * B, ["both"] * B, torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int32, device=dev)):
        assert torch.equal(model(audio=a, video=v, prompt=p, modality_mask=mask)["logits"], base)
        assert model.last_modality_modes.tolist() == [0] * B
    model(audio=a, video=v, prompt=p)
    assert model.last_modality_modes is None


def test_forward_reads_only_the_stream_a_clip_uses(dev, setup, model):
    _, _, audio, video, _, prompt = setup
    p = prompt.to(dev)
    run = lambda au, vi, mask=MIXED: model(audio=au.to(dev), video=vi.to(dev), prompt=p, modality_mask=mask)["logits"]
    ref = run(audio, video)
    assert torch.equal(run(audio, video, ["both", "audio", "video"]), ref)
    assert torch.equal(run(audio, video, torch.tensor(MIXED, dtype=torch.int32, device=dev)), ref)
    # the unused streams: clip 1's video, clip 2's audio
    assert torch.equal(run(other(audio, [2], 1), other(video, [1], 2)), ref)
    # the used streams: every clip changes, and only the clip that was touched
    for au, vi, hit in ((other(audio, [1], 3), video, 1), (audio, other(video, [2], 4), 2), (other(audio, [0], 5), video, 0), (audio, other(video, [0], 6), 0)):
        out = run(au, vi)
        for b in range(B):
            assert torch.equal(out[b], ref[b]) == (b != hit), (hit, b)
    # and the modes matter: the mixed call differs from the default call on clips 1 and 2 only
    base = model(audio=audio.to(dev), video=video.to(dev), prompt=p)["logits"]
    assert torch.equal(ref[0], base[0]) and not torch.equal(ref[1], base[1]) and not torch.equal(ref[2], base[2])


def test_encode_with_mask_vs_float64(dev, setup, model):
    _, _, audio, video, _, prompt = setup
    a, v, p = audio.to(dev), video.to(dev), prompt.to(dev)
    x, am = model.encode(a, v, p, modality_mask=MIXED)
    fa, fv, Lc = model._features(a, v)
    pe = model._embed_prompt(p)
    assert Lc == 64 and x.shape == (B, pe.shape[1] + Lc, model.llm_dim) and am.shape == x.shape[:2]
    args = (MIXED, Lc, x.shape[1], model.fusion_scale)
    ref = RM.fuse_pool_rows(fa.cpu(), fv.cpu(), pe.cpu(), *args)
    cpu = RM.fuse_pool_rows(fa.cpu(), fv.cpu(), pe.cpu(), *args, dtype=torch.float32)
    d = (x.double().cpu() - ref).abs()
    bar = Bar.fp32_bar(ref, cpu)
    print(f"encode(modality_mask): max |err| {float(d.max()):.3e}, bar {float(torch.as_tensor(bar).max()):.3e}")
    assert float((d - bar).max()) <= 0.0
    assert torch.equal(x[1, pe.shape[1]:pe.shape[1] + fa.shape[1]], fa[1])          # audio only, identity geometry: the connector's rows as they are


def padded(ids, n, pad):
    return torch.cat([ids, ids.new_full((ids.shape[0], n - ids.shape[1]), pad)], dim=1)


@pytest.mark.parametrize("kw", [{}, {"num_beams": 2, "num_return_sequences": 2}], ids=["greedy", "beams"])
def test_generate_mask_acts_per_clip(dev, setup, model, kw):
    _, _, audio, video, _, prompt = setup
    a, v = audio.to(dev), video.to(dev)
    n = kw.get("num_return_sequences", 1)
    gen = lambda mask: padded(model.generate(audio=a, video=v, max_new_tokens=8, modality_mask=mask, **kw), 8, model.tokenizer.pad_token_id)
    mixed = gen(MIXED)
    assert mixed.shape == (B * n, 8)
    uniform = {m: gen([m] * B) for m in set(MIXED)}
    for b, m in enumerate(MIXED):
        assert torch.equal(mixed[b * n:(b + 1) * n], uniform[m][b * n:(b + 1) * n]), (b, m)
    assert torch.equal(uniform[0], padded(model.generate(audio=a, video=v, max_new_tokens=8, **kw), 8, model.tokenizer.pad_token_id))


def test_train_mode_draws_and_eval_does_not(dev, setup):
    oc, W, audio, video, labels, prompt = setup
    a, v, p, lab = audio.to(dev), video.to(dev), prompt.to(dev), labels.to(dev)
    for dropout in (0.0, 0.05):           # with and without LoRA dropout the seed is that of the forward's number
        m = make_model(oc, W, "fp32", max_seq_len=64, dropout=dropout, train_connectors=False, modality_dropout_audio=0.3, modality_dropout_video=0.3)
        seen = []
        for step in (1, 2, 3, 4):
            m(audio=a, video=v, prompt=p, labels=lab)
            assert m.last_modality_seed == RM.step_seed(step)
            if dropout:
                assert m.llm_engine.desc.dropout_seed == RM.step_seed(step)
            assert m.last_modality_modes.tolist() == RM.draw(B, 0.3, 0.3, RM.step_seed(step))
            seen.append(tuple(m.last_modality_modes.tolist()))
        assert len(set(seen)) > 1
        m(audio=a, video=v, prompt=p, labels=lab, modality_mask=[1, 0, 2])               # given entries survive the draw
        assert m.last_modality_modes.tolist() == RM.draw(B, 0.3, 0.3, RM.step_seed(5), [1, 0, 2])
        m(audio=a, video=None, prompt=p, labels=lab)                                   # one stream: nothing to draw
        assert m.last_modality_modes is None
        m.eval()
        m(audio=a, video=v, prompt=p)
        assert m.last_modality_modes is None
        m.generate(audio=a, video=v, max_new_tokens=2)
        assert m.last_modality_modes is None


def test_connector_gradients_of_a_clip_without_video(dev, setup):
    """Only clip 1 is supervised and it is in mode 1: the video connector sees exact zeros, the audio connector what it sees when every clip is
    in mode 1 (bars.F32_GRAD_REL_MAX, the bar of test_connector_train_gpu.py for fp32 connector gradients)."""
    oc, W, audio, video, labels, prompt = setup
    lab = labels.clone()
    lab[0], lab[2] = -100, -100
    grads = {}
    for name, mask in (("mixed", MIXED), ("uniform", [1] * B)):
        m = make_model(oc, W, "fp32", max_seq_len=512)
        m(audio=audio.to(dev), video=video.to(dev), prompt=prompt.to(dev), labels=lab.to(dev), modality_mask=mask)["loss"].backward()
        grads[name] = conn_grads(m)
        assert m._conn_geo[-1] is m.last_modality_modes and m.last_modality_modes.tolist() == mask
    for k, g in grads["mixed"].items():
        ref = grads["uniform"][k]
        if k.startswith("video_connector"):
            assert float(g.abs().max()) == 0.0 and float(ref.abs().max()) == 0.0, k
        else:
            d = float((g - ref).abs().max())
            print(f"{k}: max |diff| {d:.3e}, max |ref| {float(ref.abs().max()):.3e}")
            assert float(ref.abs().max()) > 1e-4 and d <= Bar.F32_GRAD_REL_MAX * float(ref.abs().max()), k
    # the default call on the same labels does train the video connector
    m = make_model(oc, W, "fp32", max_seq_len=512)
    m(audio=audio.to(dev), video=video.to(dev), prompt=prompt.to(dev), labels=lab.to(dev))["loss"].backward()
    assert m._conn_geo[-1] is None and float(conn_grads(m)["video_connector.linear.weight"].abs().max()) > 0.0


def test_refusals(dev, setup, model):
    oc, W, audio, video, _, prompt = setup
    a, v = audio.to(dev), video.to(dev)
    for call in (model.forward, model.encode, model.generate):
        with pytest.raises(ValueError, match="modality_mask needs a call with both"):
            call(audio=a, video=None, modality_mask=[0] * B)
        with pytest.raises(ValueError, match="2 entries for a batch of 3"):
            call(audio=a, video=v, modality_mask=[0, 1])
        with pytest.raises(ValueError, match=r"modality_mask\[2\]"):
            call(audio=a, video=v, modality_mask=[0, 1, 3])
        with pytest.raises(ValueError, match="int32"):
            call(audio=a, video=v, modality_mask=torch.zeros(B, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="modality_dropout_audio"):
        make_model(oc, W, "fp32", modality_dropout_audio=1.2)
    with pytest.raises(ValueError, match="at most 1"):
        make_model(oc, W, "fp32", modality_dropout_audio=0.7, modality_dropout_video=0.4)
    with pytest.raises(ValueError, match="needs modality='both'"):
        make_model(oc, W, "fp32", train_connectors=False, modality="audio", modality_dropout_video=0.1)
