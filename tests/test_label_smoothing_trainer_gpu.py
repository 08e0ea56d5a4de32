"""label_smoothing / z_loss through ClipWhisperTrainer on the tiny golden model of tests/test_label_smoothing_model_gpu.py at (0.1, 1e-3), fp32 and
bf16: the captured graph against the eager step; a grad_accum_steps = 2 window of 2 x 1 clips against the one-batch step of the same two clips
(and, in bf16, against host autograd under the same objective) at the bars of tests/test_grad_accum_trainer_gpu.py; last_nll; the checkpoint's
metadata.  One process, every step on one stream."""
import json
import logging
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import connector_expect as CE  # noqa: E402
from test_connector_train_gpu import make_model  # noqa: E402
from test_label_smoothing_model_gpu import EPS, Z, batch, expectation  # noqa: E402,F401  (batch: the module's fixture)


def make(batch, precision, graph=False, N=1, eps=EPS, z=Z, **kw):
    from avllm.trainer import ClipWhisperTrainer
    oc, W, *_ = batch
    m = make_model(oc, W, precision, label_smoothing=eps, z_loss=z)
    tr = ClipWhisperTrainer(m, learning_rate=1e-3, weight_decay=0.01, grad_clip=0.5, total_steps=10, max_epochs=1, use_graph=graph,
                            grad_accum_steps=N, **kw)
    return m, tr


def feed(tr, batch, idx=(0, 1)):
    _, _, audio, video, lab, prompt = batch
    idx = list(idx)
    return tr.train_step(audio[idx].cuda(), video[idx].cuda(), lab[idx].cuda(), prompt[idx].cuda())


def same_loss(a, b, rows=48):
    """test_connector_train_gpu.same_loss: two runs of one step differ by the order of avllm_ce_smooth_fwd's float atomics alone."""
    return abs(a - b) <= Bar.atomic_sum_term(rows, max(abs(a), abs(b)))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graph_replay_equals_eager(dev, batch, precision):
    runs = []
    for graph in (False, True):
        m, tr = make(batch, precision, graph=graph)
        steps = []
        for _ in range(3):
            loss = float(feed(tr, batch))
            steps.append((loss, float(tr.last_nll)))
        runs.append((m, tr, steps))
    (m0, t0, s0), (m1, t1, s1) = runs
    assert any(isinstance(v, dict) for v in t1._graphs.values())              # step 2 captured, step 3 replayed
    assert all(same_loss(a[0], b[0]) and same_loss(a[1], b[1]) for a, b in zip(s0, s1)), (s0, s1)
    assert torch.equal(m0.llm_engine.lora_p, m1.llm_engine.lora_p) and torch.equal(m0.conn_p, m1.conn_p)
    assert torch.equal(t0.m, t1.m) and torch.equal(t0.v, t1.v) and torch.equal(t0.cm, t1.cm) and torch.equal(t0.cv, t1.cv)
    assert s0[0][0] != s0[2][0]                                               # the parameters moved


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_window_of_two_micro_batches_equals_the_one_batch_step(dev, batch, precision, graph):
    m1, t1 = make(batch, precision)
    l1 = float(feed(t1, batch))
    g1 = {"lora_g": m1.llm_engine.lora_g.clone(), "conn_g": m1.conn_g.clone()}
    m, tr = make(batch, precision, graph=graph, N=2)
    micro = [float(feed(tr, batch, (i,))) for i in (0, 1)]
    assert tr.micro_step == 0 and tr.global_step == 1
    wl, got = float(tr.window_loss), tr.window_gradients()
    print(f"{precision} window loss {wl:.7f}, one batch {l1:.7f}, micro-batches {micro}")
    views = {"lora_g": m.llm_engine.lora_views, "conn_g": lambda b: dict(zip(CE.CONNECTOR_KEYS, m.connector_grad_views(b)))}
    if precision == "fp32":
        assert abs(wl - l1) < Bar.F32_LOSS_ABS
        for k in ("lora_g", "conn_g"):
            for (name, a), b in zip(views[k](got[k]).items(), views[k](g1[k]).values()):
                d, mx = float((a - b).abs().max()), float(b.abs().max())
                assert d <= Bar.F32_GRAD_REL_MAX * mx, (name, d, mx)
    else:
        ref_loss, _, ref_cg, ref_lg = expectation(batch, EPS, Z)
        flat = {"lora_g": torch.zeros(got["lora_g"].numel()), "conn_g": torch.zeros(got["conn_g"].numel())}
        for k, view in m.llm_engine.lora_views(flat["lora_g"]).items():
            view.copy_(ref_lg[k])
        for view, k in zip(m.connector_grad_views(flat["conn_g"]), CE.CONNECTOR_KEYS):
            view.copy_(ref_cg[k])
        for what, rl, rg in (("one batch", l1, g1), ("host autograd", float(ref_loss), flat)):
            assert abs(wl - rl) < Bar.BF16_LOSS_ABS, what
            for k in ("lora_g", "conn_g"):
                r = Bar.rel_l2(got[k].cpu(), rg[k].cpu())
                print(f"bf16 {k} against {what}: rel L2 {r:.3e}")
                assert r < Bar.BF16_GRAD_REL_L2, (what, k, r)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_last_nll_and_checkpoint_metadata(dev, batch, precision, tmp_path, caplog):
    m, tr = make(batch, precision, output_dir=str(tmp_path))
    eng = m.llm_engine
    for _ in range(STEPS):
        loss = float(feed(tr, batch))
    nll = float(tr.last_nll)
    # what the step reported is the rule on the raw sums it left behind: loss = ((1 - eps) sum nll + eps sum u + z sum q) / count, up to the four
    # sums' atomics (loss_sum adds the rows' composite terms, loss_terms their parts) and the six roundings of a row's composite term
    cnt = float(eng.acc[1])
    s_nll, s_u, s_q = (float(t) for t in eng.loss_terms)
    composite = ((1.0 - EPS) * s_nll + EPS * s_u + Z * s_q) / cnt
    tol = (Bar.atomic_sum_term(cnt, composite * cnt) + sum(Bar.atomic_sum_term(cnt, w * s) for w, s in ((1.0 - EPS, s_nll), (EPS, s_u), (Z, s_q)))) / cnt \
        + 8.0 * Bar.U32 * ((1.0 - EPS) * s_nll + EPS * s_u + Z * s_q) / cnt
    print(f"{precision}: loss {loss:.6f}, composite of the raw sums {composite:.6f} (tol {tol:.2e}), nll {nll:.6f}, mean u {s_u / cnt:.6f}, mean q {s_q / cnt:.4f}")
    assert abs(loss - composite) <= tol
    assert abs(nll - s_nll / cnt) <= Bar.U32 * nll
    # loss - nll = eps (u - nll) + z q is positive once the targets are more probable than the row's geometric-mean class (nll < u).  The seeded
    # random model starts the other way round (nll 6.46 against u = 6.04 at ln 256 = 5.55), one update of this batch turns it (nll 5.63,
    # u = 6.01), and the third step's figures are the ones judged
    assert nll == nll and abs(nll) != float("inf") and nll < loss
    tr._save_checkpoint(0, "ck.pt")
    path = os.path.join(str(tmp_path), "ck.pt")
    meta = json.load(open(path.replace(".pt", "_meta.json")))
    assert meta["label_smoothing"] == EPS and meta["z_loss"] == Z
    assert tr.checkpoint_loss_options(path) == (EPS, Z)
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        _, same = make(batch, precision)
        same.load_checkpoint(path)
        assert not [r for r in caplog.records if "label_smoothing" in r.getMessage()]
        other_m, other = make(batch, precision, eps=0.0, z=0.0)
        other.load_checkpoint(path)                                           # warns and goes on
        assert [r for r in caplog.records if "label_smoothing=0.1" in r.getMessage() and "z_loss=0.001" in r.getMessage()]
    assert other.last_nll is None and other.global_step == STEPS
    assert torch.equal(other_m.llm_engine.lora_p, m.llm_engine.lora_p)


STEPS = 3
