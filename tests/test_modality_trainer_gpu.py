"""Modality dropout in the trainer (tiny golden model, train_connectors=True): the draw sits inside the captured step after step_advance, so
a replayed graph redraws from the step's device seed -- graph replay == eager in modes, losses, parameters and moments, mirroring
test_connector_train_gpu.py::test_graph_replay_equals_eager_with_connectors -- and probabilities of zero are the model without the keywords."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import refs64_modality as RM  # noqa: E402
from test_connector_train_gpu import batch_for, make_model, same_loss, tiny  # noqa: E402,F401  (tiny: the module-scoped fixture)

P_DROP = (0.3, 0.3)


def run(tiny, dev, graph, steps=3, **model_kw):
    from avllm.trainer import ClipWhisperTrainer
    oc2, W, audio, video, lab, prompt = batch_for(tiny, "pool")
    m = make_model(oc2, W, "fp32", dropout=0.05, **model_kw)
    tr = ClipWhisperTrainer(m, learning_rate=1e-3, total_steps=10, max_epochs=1, grad_clip=0.5, use_graph=graph)
    losses, modes = [], []
    for _ in range(steps):
        losses.append(float(tr.train_step(audio.to(dev), video.to(dev), lab.to(dev), prompt.to(dev))))
        modes.append(None if m.last_modality_modes is None else tuple(m.last_modality_modes.tolist()))
    return m, tr, losses, modes


def test_graph_replay_redraws_and_equals_eager(dev, tiny):
    kw = dict(modality_dropout_audio=P_DROP[0], modality_dropout_video=P_DROP[1])
    m0, t0, l0, modes0 = run(tiny, dev, False, **kw)
    m1, t1, l1, modes1 = run(tiny, dev, True, **kw)
    assert any(isinstance(v, dict) for v in t1._graphs.values())          # step 2 captured, step 3 replayed
    want = [tuple(RM.draw(2, *P_DROP, RM.step_seed(s))) for s in (1, 2, 3)]
    assert modes0 == want and modes1 == want, (modes0, modes1, want)
    assert len(set(want)) == 3                                            # the draw is not frozen into the graph (pinned on the CPU too)
    assert all(same_loss(a, b) for a, b in zip(l0, l1)), (l0, l1)
    assert torch.equal(m0.conn_p, m1.conn_p) and torch.equal(m0.llm_engine.lora_p, m1.llm_engine.lora_p)
    assert torch.equal(t0.cm, t1.cm) and torch.equal(t0.cv, t1.cv) and torch.equal(t0.m, t1.m) and torch.equal(t0.v, t1.v)
    shares = t1.mode_shares(torch.tensor(sum(modes1, ())))
    assert shares == [4 / 6, 0.0, 2 / 6]
    # and the modes did act: the same three steps without modality dropout end elsewhere
    m2, *_ = run(tiny, dev, True)
    assert not torch.equal(m2.conn_p, m1.conn_p)


def test_zero_probabilities_are_the_model_without_the_keywords(dev, tiny):
    m0, t0, l0, modes0 = run(tiny, dev, True)
    m1, t1, l1, modes1 = run(tiny, dev, True, modality_dropout_audio=0.0, modality_dropout_video=0.0)
    assert modes0 == [None] * 3 and modes1 == [None] * 3
    assert torch.equal(m0.conn_p, m1.conn_p) and torch.equal(m0.llm_engine.lora_p, m1.llm_engine.lora_p)
    assert torch.equal(t0.cm, t1.cm) and torch.equal(t0.m, t1.m)
