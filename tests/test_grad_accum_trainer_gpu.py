"""grad_accum_steps = N on the GPU (tiny golden model): a window of N micro-batches is ONE optimizer step on their concatenation.  The yardstick
is the existing one-batch step (grad_accum_steps = 1) on the concatenated batch, and for bf16 also the CPU oracle on it (tests/connector_expect.py),
so that the bar measures distance from the reference and not from a sibling rounding.  Bars: tests/bars.py and the figures of
tests/test_connector_train_gpu.py::test_trainer_three_steps_vs_oracle (update relative to its own size < 2e-2, loss within 2e-4 in fp32).
The batch is that of tests/test_connector_ddp_gpu.py::_build: 4 clips, one row's tail padded, so the micro-batches hold different numbers of scored
tokens and a mean of per-micro-batch means would miss the bars."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import connector_expect as CE  # noqa: E402
import test_connector_train_gpu as T  # noqa: E402
from oracle import weights as Wt  # noqa: E402

ALL = [0, 1, 2, 3]
SPLITS = {"2x2": [[0, 1], [2, 3]], "4x1": [[0], [1], [2], [3]]}
_CACHE = {}


def data():
    if "data" not in _CACHE:
        oc = Wt.tiny()
        W = Wt.all_weights(oc, 0, lora_b_std=0.05)
        audio, video, labels, prompt = Wt.synthetic_batch(oc, 4, 3, seed=77)
        labels = labels[:, :24].contiguous()
        labels[0, 12:] = oc.pad_token_id                    # uneven numbers of scored tokens between the micro-batches
        _CACHE["data"] = (oc, W, audio, video, labels, prompt)
    return _CACHE["data"]


def make(precision, conn, N=None, graph=False, dropout=0.0, **kw):
    from avllm.trainer import ClipWhisperTrainer
    oc, W = data()[:2]
    m = T.make_model(oc, W, precision, dropout=dropout, train_connectors=conn)
    if N is not None:
        kw["grad_accum_steps"] = N
    kw.setdefault("total_steps", 10)
    return m, ClipWhisperTrainer(m, learning_rate=1e-3, weight_decay=0.01, grad_clip=0.5, max_epochs=1, use_graph=graph, **kw)


def feed(tr, idx, audio=None):
    _, _, a, v, lab, pr = data()
    a = a if audio is None else audio
    return tr.train_step(a[idx].cuda(), v[idx].cuda(), lab[idx].cuda(), pr[idx].cuda())


def params(m, tr):
    out = {"lora_p": m.llm_engine.lora_p.clone(), "m": tr.m.clone(), "v": tr.v.clone()}
    if tr.train_connectors:
        out.update(conn_p=m.conn_p.clone(), cm=tr.cm.clone(), cv=tr.cv.clone())
    return out


def one_batch_reference(precision, conn):
    """Two one-batch steps on all 4 clips with the existing path: loss and raw gradient of step 1, loss of step 2, parameters before and after."""
    key = ("ref", precision, conn)
    if key not in _CACHE:
        m, tr = make(precision, conn, N=1)
        init = params(m, tr)
        l1 = float(feed(tr, ALL))
        g1 = {"lora_g": m.llm_engine.lora_g.clone(), "conn_g": m.conn_g.clone() if conn else None}
        l2 = float(feed(tr, ALL))
        _CACHE[key] = (l1, g1, l2, init, params(m, tr))
    return _CACHE[key]


def oracle_reference(m):
    """The CPU oracle's loss and gradients on the concatenated batch, laid out like lora_g / conn_g."""
    if "oracle" not in _CACHE:
        oc, W, audio, video, labels, prompt = data()
        _CACHE["oracle"] = CE.connector_step(W, oc, audio, video, prompt, labels)
    loss, _, cg, lg = _CACHE["oracle"]
    flat = torch.zeros(m.llm_engine.lora_g.numel())
    for k, view in m.llm_engine.lora_views(flat).items():
        view.copy_(lg[k])
    conn = None
    if getattr(m, "train_connectors", False):
        conn = torch.zeros(m.conn_g.numel())
        for view, k in zip(m.connector_grad_views(conn), CE.CONNECTOR_KEYS):
            view.copy_(cg[k])
    return float(loss), {"lora_g": flat, "conn_g": conn}


def rel_update(have, ref, init):
    return float((have.double() - ref.double()).norm() / (ref.double() - init.double()).norm())


def same_loss(a, b, rows=4 * 24):
    return abs(a - b) <= Bar.atomic_sum_term(rows, max(abs(a), abs(b)))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("split", ["2x2", "4x1"])
@pytest.mark.parametrize("conn", [False, True], ids=["lora", "connectors"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_window_equals_the_concatenated_batch(dev, precision, conn, split, graph):
    """Window 1: loss and window_gradients() against the one-batch step.  Window 2: the update of two windows against two one-batch steps.
    fp32: the update error relative to the update is below 2e-2 and the loss within 2e-4, test_trainer_three_steps_vs_oracle's bars.
    bf16: that test and its 2e-2 are fp32 only, and two early Adam steps are sign-like -- an element whose gradient is below the bf16 noise
    moves the other way by a full lr -- so two bf16 runs that round at different points differ by more than 2e-2 of the update whatever the
    code does.  The bound is therefore taken from the existing, unchanged one-batch bf16 step (N = 1), not from the code under test: against
    the fp32 one-batch update that step is off by e1 (relative to the fp32 update), which is what bf16 does to two steps of this model; the
    windowed bf16 run is the same computation rounded at other points (the backward carries the sum instead of the mean, the connector
    gradient is added in two or four parts), i.e. another draw of the same error, and must stay within 2 x e1 against the same fp32
    reference -- the factor bars.py allows between an estimate of a bf16 error and its bar.  A wrong divisor, clip, pack_lora or connector
    refresh in the closing part moves the update by its own size, far beyond that.  The loss of window 2 is held to BF16_LOSS_ABS."""
    l1, g1, l2, init, final = one_batch_reference(precision, conn)
    parts = SPLITS[split]
    m, tr = make(precision, conn, N=len(parts), graph=graph)
    assert tr.micro_step == 0 and tr.global_step == 0
    for j, idx in enumerate(parts):
        assert tr.micro_step == j
        feed(tr, idx)
    assert tr.micro_step == 0 and tr.global_step == 1
    wl, got = float(tr.window_loss), tr.window_gradients()
    assert (got["conn_g"] is not None) == conn
    if precision == "fp32":
        print(f"fp32 {split} window loss {wl:.7f}, one batch {l1:.7f}")
        assert abs(wl - l1) < Bar.F32_LOSS_ABS
        for k in ("lora_g", "conn_g"):
            if got[k] is None:
                continue
            views = m.llm_engine.lora_views if k == "lora_g" else (lambda b: dict(zip(CE.CONNECTOR_KEYS, m.connector_grad_views(b))))
            for (name, a), b in zip(views(got[k]).items(), views(g1[k]).values()):
                d, mx = float((a - b).abs().max()), float(b.abs().max())
                assert d <= Bar.F32_GRAD_REL_MAX * mx, (name, d, mx)
    else:
        ol, og = oracle_reference(m)
        for what, rl, rg in (("one batch", l1, g1), ("oracle", ol, og)):
            print(f"bf16 {split} window loss {wl:.5f}, {what} {rl:.5f}")
            assert abs(wl - rl) < Bar.BF16_LOSS_ABS, what
            for k in ("lora_g", "conn_g"):
                if got[k] is not None:
                    r = Bar.rel_l2(got[k].cpu(), rg[k].cpu())
                    print(f"bf16 {split} {k} against {what}: rel L2 {r:.3e}")
                    assert r < Bar.BF16_GRAD_REL_L2, (what, k, r)
    for idx in parts:
        feed(tr, idx)
    assert tr._sync_step() == 2
    have = params(m, tr)
    wl2 = float(tr.window_loss)
    _, _, _, init32, final32 = one_batch_reference("fp32", conn)
    for k in ("lora_p", "conn_p") if conn else ("lora_p",):
        r = rel_update(have[k], final[k], init[k])
        print(f"{precision} {split} {k}: two windows against two one-batch steps, update error / update {r:.3e}")
        if precision == "fp32":
            assert r < 2e-2, (k, r)
        else:
            assert torch.equal(init[k], init32[k])                          # fp32 masters: both precisions start from the same bits
            e1, ew = rel_update(final[k], final32[k], init32[k]), rel_update(have[k], final32[k], init32[k])
            print(f"bf16 {split} {k}: against the fp32 one-batch update, one-batch bf16 {e1:.3e}, windowed bf16 {ew:.3e}, bar {2 * e1:.3e}")
            assert ew <= 2.0 * e1, (k, ew, e1)
    assert abs(wl2 - l2) < (2e-4 if precision == "fp32" else Bar.BF16_LOSS_ABS), (wl2, l2)


def test_fp8_window_equals_the_one_batch_step(dev):
    m0, t0 = make("fp8", False, N=1)
    l0 = float(feed(t0, ALL))
    g0 = m0.llm_engine.lora_g.clone()
    m, tr = make("fp8", False, N=2)
    for idx in SPLITS["2x2"]:
        feed(tr, idx)
    r = Bar.rel_l2(tr.window_gradients()["lora_g"].cpu(), g0.cpu())
    print(f"fp8 window gradient against the one-batch fp8 step: rel L2 {r:.3e}; loss {float(tr.window_loss):.5f} against {l0:.5f}")
    assert r < Bar.BF16_GRAD_REL_L2 and abs(float(tr.window_loss) - l0) < Bar.BF16_LOSS_ABS


def test_it_really_accumulates(dev):
    """After micro-step 0 of N = 2 nothing an optimizer step writes has moved; after micro-step 1 everything has.  The device word state.step
    is NOT bit-equal after micro-step 0, by design: avllm_step_advance_micro advances step, lr and the bias corrections at micro-step 0 (the
    window's lr and dropout seeds are needed from its first forward on), so the word already counts the step the open window will take.
    What stays put is the number of optimizer steps TAKEN, which _sync_step() reads as step minus one while a window is open."""
    m, tr = make("fp32", True, N=2)
    before = params(m, tr)
    state0 = tr.state.cpu().clone()
    feed(tr, [0, 1])
    assert all(torch.equal(v, params(m, tr)[k]) for k, v in before.items()), "a micro-step that does not close the window moved something"
    assert tr.global_step == 0 and tr.micro_step == 1 and tr._sync_step() == 0
    feed(tr, [2, 3])
    after = params(m, tr)
    assert all(not torch.equal(v, after[k]) for k, v in before.items())
    assert not torch.equal(state0, tr.state.cpu())
    lr1 = float(tr.state.cpu().numpy().view(np.float32)[2])
    for idx in SPLITS["2x2"]:
        feed(tr, idx)
    assert tr._sync_step() == 2 and tr.global_step == 2
    lr2 = float(tr.state.cpu().numpy().view(np.float32)[2])
    assert abs(lr1 - tr.lr_at(0)) < 1e-9 and abs(lr2 - tr.lr_at(1)) < 1e-9 and lr1 != lr2          # the schedule ticked once per window


def test_partial_window_and_flush(dev):
    """3 micro-batches at N = 2, then flush(): the second update is a one-batch step on the third micro-batch alone."""
    m, tr = make("fp32", True, N=2)
    feed(tr, [0, 1]); feed(tr, [2])
    mid = params(m, tr)
    feed(tr, [3])
    assert tr.micro_step == 1 and tr.flush() is not None and tr.micro_step == 0 and tr.global_step == 2
    got, wl = tr.window_gradients(), float(tr.window_loss)
    # the yardstick: a one-batch trainer put into the same state, stepping on clip 3
    m1, t1 = make("fp32", True, N=1)
    m1.llm_engine.lora_p.copy_(mid["lora_p"]); m1.conn_p.copy_(mid["conn_p"])
    m1.llm_engine.pack_lora(); m1.refresh_connectors()
    t1.m.copy_(mid["m"]); t1.v.copy_(mid["v"]); t1.cm.copy_(mid["cm"]); t1.cv.copy_(mid["cv"])
    t1.state.view(torch.int32)[0] = 1
    l1 = float(feed(t1, [3]))
    assert abs(wl - l1) < Bar.F32_LOSS_ABS
    for a, b in ((got["lora_g"], m1.llm_engine.lora_g), (got["conn_g"], m1.conn_g)):
        assert float((a - b).abs().max()) <= Bar.F32_GRAD_REL_MAX * float(b.abs().max())
    have = params(m, tr)
    for k in ("lora_p", "conn_p"):
        assert rel_update(have[k], params(m1, t1)[k], mid[k]) < 2e-2, k
    state = tr.state.cpu().clone()
    assert tr.flush() is None                               # nothing pending: nothing happens
    assert all(torch.equal(v, params(m, tr)[k]) for k, v in have.items()) and torch.equal(state, tr.state.cpu())


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_nonfinite_window_touches_nothing_and_counts_once(dev, graph):
    """Windows (good, BAD), (good, good) against a run that never saw the bad window: the form of
    test_connector_train_gpu.py::test_nonfinite_batch_touches_nothing_and_counts_once."""
    audio = data()[2]
    bad_audio = audio.clone()
    bad_audio[2, 0, 0] = float("nan")
    runs = []
    good = ((audio, [0, 1]), (audio, [2, 3])) * 2
    for seq in (((audio, [0, 1]), (bad_audio, [2, 3])) + good, good):
        m, tr = make("fp32", True, N=2, graph=graph, warmup_steps=2)
        for j, (a, idx) in enumerate(seq):
            before = params(m, tr)
            loss = feed(tr, idx, audio=a)
            if a is bad_audio:
                assert not bool(torch.isfinite(loss)) and not bool(torch.isfinite(tr.window_loss))
                assert all(torch.equal(v, params(m, tr)[k]) for k, v in before.items())
        runs.append((m, tr))
    (m, tr), (mr, trr) = runs
    assert tr.skipped_steps == 1 and trr.skipped_steps == 0 and tr._sync_step() == 2 == trr._sync_step()
    assert float(tr.state.cpu().numpy().view(np.float32)[5]) == 1.0                          # state.skipped: once per bad window
    assert torch.equal(tr.state.cpu()[8:20], trr.state.cpu()[8:20])                          # lr, bc1, bc2_sqrt of the last step
    assert int(tr.state.view(torch.int32)[6]) == 0
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    assert rel(m.conn_p, mr.conn_p) < 1e-5 and rel(m.llm_engine.lora_p, mr.llm_engine.lora_p) < 1e-5


def test_micro_batches_draw_their_own_dropout_masks(dev):
    runs = []
    for _ in range(2):
        m, tr = make("fp32", False, N=2, dropout=0.05)
        runs.append([float(feed(tr, [0, 1])), float(feed(tr, [0, 1]))])
    (a0, a1), (b0, b1) = runs
    assert a0 != a1, "the two micro-batches of a window drew the same masks"
    assert same_loss(a0, b0) and same_loss(a1, b1), runs


def test_graph_replay_equals_eager_over_mixed_windows(dev):
    """3 windows of N = 2, two input signatures alternating inside every window: parameters and moments bit-equal, losses up to same_loss."""
    runs = []
    for graph in (False, True):
        m, tr = make("fp32", True, N=2, graph=graph, dropout=0.05)
        losses = []
        for _ in range(3):
            losses.append(float(feed(tr, [0, 1])))
            losses.append(float(feed(tr, [2])))
            losses.append(float(tr.window_loss))
        runs.append((m, tr, losses))
    (m0, t0, l0), (m1, t1, l1) = runs
    assert sum(isinstance(v, dict) for v in t1._graphs.values()) == 2 and isinstance(t1._close_graph, tuple)
    assert all(same_loss(a, b) for a, b in zip(l0, l1)), (l0, l1)
    p0, p1 = params(m0, t0), params(m1, t1)
    assert all(torch.equal(p0[k], p1[k]) for k in p0)
    assert t0._sync_step() == 3 == t1._sync_step()


def test_checkpoint_at_window_boundaries(dev, tmp_path):
    windows = lambda tr, n: [float(feed(tr, idx)) for _ in range(n) for idx in SPLITS["2x2"]]
    m_full, t_full = make("fp32", True, N=2, dropout=0.05)
    windows(t_full, 3)
    m_a, t_a = make("fp32", True, N=2, dropout=0.05, output_dir=str(tmp_path))
    windows(t_a, 1)
    feed(t_a, [0, 1])
    t_a._save_checkpoint(0, "ck.pt")                         # asked for mid-window: waits for the boundary
    assert not os.path.exists(os.path.join(str(tmp_path), "ck.pt"))
    feed(t_a, [2, 3])
    assert os.path.exists(os.path.join(str(tmp_path), "ck.pt"))
    meta = json.load(open(os.path.join(str(tmp_path), "ck_meta.json")))
    assert meta["grad_accum_steps"] == 2 and meta["global_step"] == 2
    m_b, t_b = make("fp32", True, N=2, dropout=0.05)
    t_b.load_checkpoint(os.path.join(str(tmp_path), "ck.pt"))
    assert t_b.micro_step == 0 and t_b.global_step == 2
    windows(t_b, 1)
    pf, pb = params(m_full, t_full), params(m_b, t_b)
    assert all(torch.equal(pf[k], pb[k]) for k in ("lora_p", "conn_p"))


@pytest.mark.parametrize("tail", ["batch", "skipped batch"])
def test_epoch_closes_its_last_partial_window(dev, tail, caplog):
    """_train_epoch over 3 batches at N = 2: two optimizer steps (the second on the third batch alone, by flush()), nothing pending afterwards,
    and the default schedule length counts windows.  With a malformed batch after them the epoch ends on a skipped batch: the open window is
    closed after the loop, and is counted into the average and logged like the first."""
    import logging
    from avllm.trainer import ClipWhisperTrainer
    _, _, a, v, lab, pr = data()
    loader = [{"audio": a[i].cuda(), "video": v[i].cuda(), "labels": lab[i].cuda(), "prompt": pr[i].cuda()} for i in ([0, 1], [2], [3])]
    if tail == "skipped batch":
        loader.append("garbage")                            # _unpack raises on it: logged and skipped
    m = T.make_model(*data()[:2], "fp32", train_connectors=False)
    tr = ClipWhisperTrainer(m, train_dataloader=loader, max_epochs=2, learning_rate=1e-3, grad_accum_steps=2, log_interval=1)
    assert tr.total_steps == 4
    with caplog.at_level(logging.INFO):
        avg = tr._train_epoch(0)
    assert tr.micro_step == 0 and tr._sync_step() == 2 and tr.global_step == 2
    lines = [r.getMessage() for r in caplog.records if " loss " in r.getMessage()]
    assert len(lines) == 2 and "window 1 " in lines[0] and "window 2 " in lines[1], lines
    m1, t1 = make("fp32", False, N=2)
    feed(t1, [0, 1]); feed(t1, [2]); w1 = float(t1.window_loss)
    feed(t1, [3]); t1.flush(); w2 = float(t1.window_loss)
    assert abs(avg - (w1 + w2) / 2) < 1e-4, (avg, w1, w2)


def test_abandoned_window_leaves_no_trace(dev):
    """What _train_epoch does when a micro-step raises: the open window is given up, the step it started is taken back, and the next window is
    that of a run that never saw it."""
    runs = []
    for abandon in (True, False):
        m, tr = make("fp32", True, N=2)
        if abandon:
            feed(tr, [2, 3])
            assert tr._abandon_window() == 1 and tr.micro_step == 0 and tr._sync_step() == 0
        for idx in SPLITS["2x2"]:
            feed(tr, idx)
        runs.append((params(m, tr), tr.state.cpu().clone(), float(tr.window_loss)))
    (pa, sa, la), (pb, sb, lb) = runs
    assert torch.equal(sa, sb) and same_loss(la, lb)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    assert all(rel(pa[k], pb[k]) < 1e-5 for k in ("lora_p", "conn_p"))


def test_one_is_the_path_without_the_keyword(dev):
    runs = []
    for N in (1, None):
        m, tr = make("fp32", True, N=N, graph=True, dropout=0.05)
        for _ in range(3):
            feed(tr, ALL)
        runs.append((params(m, tr), tr.state.cpu().clone()))
        assert not hasattr(tr, "_window")                    # no new allocation on this path
    (p0, s0), (p1, s1) = runs
    assert all(torch.equal(p0[k], p1[k]) for k in p0) and torch.equal(s0, s1)
