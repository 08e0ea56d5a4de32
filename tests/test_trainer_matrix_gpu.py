"""ClipWhisperTrainer.train_step() on the GPU across the case list of tests/trainer_cases.py (tiny golden model): from a batch to the updated
parameters -- augmentation, encoders, modality draw, fusion, loss, backward, connector backward, window sums, one clip, one AdamW step, the
schedule -- against the host restatement tests/refs64_trainer.py.

Every optimizer step is judged TEACHER-FORCED: the restatement starts from the parameters, moments and device step state read back before the
step, so nothing compounds.  Per step trainer_cases.ratios compares the modes of every micro-batch (equal), the augmented inputs (pixels by
bits, features by bits or at the log-mel bar; for a replayed graph what the step consumed is read from static_inputs), the window loss and the
pre-clip gradient (fp32: bars.F32_LOSS_ABS, bars.F32_GRAD_REL_MAX per tensor; bf16: bars.BF16_LOSS_ABS, bars.BF16_GRAD_REL_L2 over the LoRA
gradient and over the connector gradient, as tests/test_connector_train_gpu.py and tests/test_grad_accum_trainer_gpu.py judge them), and the
update: parameters and moments against the float64 clip + AdamW rule on the DEVICE's own pre-clip gradient, moments, count and schedule record
at tests/test_bytemovers_gpu.py's AdamW bar (AdamW's first steps are near sign-like and would amplify a gradient difference that is within its
bar; the gradient is judged on its own).  The device's sum of squares is first held to that file's grad_sumsq bar against the float64 sum over
its own gradient buffers, then used for the clip coefficient (the fp32 yardstick of bars.fp32_bar forms its coefficient in fp32, where
that file's test_adamw hands one float64 coefficient to both rules: trainer_cases.ratios), and the rule takes beta1, beta2, eps and the decay as the kernel's float arguments hold them: what is left to the AdamW
bar is the arithmetic of the rule (trainer_cases.ratios says how).  Every ratio is printed; a case passes when none exceeds 1.

The schedule record of every step (lr, bc1, bc2_sqrt) is compared with refs64.schedule at the count of steps taken, at the bar of
tests/test_bytemovers_gpu.py::test_step_advance; four cases run under a warm-up.

Events: a non-finite window leaves parameters, moments and step count bit-identical and skipped_steps one higher; a trainer loaded from the
checkpoint takes its next step with the modes, augmented inputs, parameters and moments of the trainer that went on, bit for bit, and the same
loss up to bars.atomic_sum_term (avllm_ce_fwd adds the rows' terms with float atomics in arrival order: two runs of one step do not report the
same bits, tests/test_connector_train_gpu.py::same_loss)."""
import math
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import connector_expect as CE  # noqa: E402
import refs64_augment as RA  # noqa: E402
import refs64_trainer as RT  # noqa: E402
import trainer_cases as TC  # noqa: E402


def build(c, out_dir, dev="cuda:0", **trainer_kw):
    from avllm.preprocess import AudioAugment, NoiseBank, VideoAugment
    from avllm.trainer import ClipWhisperTrainer
    from test_connector_train_gpu import make_model
    oc, W = TC.pool()[:2]
    kw = {} if c.moddrop is None else dict(modality_dropout_audio=c.moddrop[0], modality_dropout_video=c.moddrop[1])
    m = make_model(oc, W, c.precision, dropout=c.drop, train_connectors=bool(c.conn), **kw)
    aa = va = None
    if c.audio_aug is not None:
        a = c.audio_aug
        aa = AudioAugment(noise=None if a["noise"] is None else NoiseBank(a["noise"], dev), snr_db=a["snr_db"], noise_prob=a["noise_prob"],
                          time_masks=a["time_masks"], time_width=a["time_width"], time_ratio=a["time_ratio"], freq_masks=a["freq_masks"],
                          freq_width=a["freq_width"], fill=a["fill"])
    if c.video_aug is not None:
        v = c.video_aug
        va = VideoAugment(resize=v["resize"], random_crop=v["random_crop"], flip_prob=v["flip_prob"], time_masks=v["time_masks"],
                          time_width=v["time_width"], time_ratio=v["time_ratio"], fill=v["fill"])
    h = c.hyper
    trainer_kw.setdefault("use_graph", c.graph)
    trainer_kw.setdefault("bwd_pieces", c.pieces)
    tr = ClipWhisperTrainer(m, learning_rate=h.lr, weight_decay=h.weight_decay, grad_clip=h.grad_clip, max_epochs=1, total_steps=h.total_steps,
                            warmup_steps=h.warmup_steps, grad_accum_steps=c.N, audio_augment=aa, video_augment=va, augment_seed=h.augment_seed,
                            output_dir=str(out_dir), **trainer_kw)
    return m, tr


def as_dict(m, c, lora_flat, conn_flat):
    d = {"lora." + k: v.double().clone() for k, v in m.llm_engine.lora_views(lora_flat.detach().cpu()).items()}
    if c.conn:
        d.update({k: v.double().clone() for k, v in zip(CE.CONNECTOR_KEYS, m.connector_grad_views(conn_flat.detach().cpu()))})
    return d


def read_state(m, tr, c):
    """Parameters, moments and the device step record, as tests/refs64_trainer.py's fields."""
    from avllm import lib as L
    st = L.StepState.from_buffer_copy(bytes(tr.state.cpu().numpy().tobytes()))
    conn = (m.conn_p, tr.cm, tr.cv) if c.conn else (None, None, None)
    return SimpleNamespace(par=as_dict(m, c, m.llm_engine.lora_p, conn[0]), mo=as_dict(m, c, tr.m, conn[1]), vo=as_dict(m, c, tr.v, conn[2]),
                           step=int(st.step), skipped=int(st.skipped), lr=float(st.lr), bc1=float(st.bc1), bc2_sqrt=float(st.bc2_sqrt),
                           open_micro=int(st.reserved[0]))


def run_window(m, tr, c, window, w, after_first_micro=None):
    """One optimizer step of the trainer on `window`, read back into the fields trainer_cases.ratios compares."""
    modes, inputs = [], []
    loss = None
    for j, (idx, bad) in enumerate(window):
        assert tr._augment_index() == w * c.N + j and tr.micro_step == (j if c.N > 1 else 0)
        unpacked = tr._unpack(TC.trainer_batch(c, idx, bad))
        loss = tr.train_step(*unpacked)
        static = tr.static_inputs(*unpacked)
        a, v = (static[0], static[1]) if static is not None else (unpacked[0], unpacked[1])      # a replayed graph: what the step consumed
        assert static is None or (TC._same_bits(static[0].cpu(), unpacked[0].cpu()) and TC._same_bits(static[1].cpu(), unpacked[1].cpu()))
        inputs.append((a.detach().float().cpu(), v.detach().float().cpu()))
        modes.append(None if m.last_modality_modes is None else m.last_modality_modes.tolist())
        if j == 0 and after_first_micro is not None:
            after_first_micro()
    if c.N > 1 and tr.micro_step > 0:
        assert len(window) < c.N and tr.flush() is not None
    assert tr.micro_step == 0
    after = read_state(m, tr, c)
    assert after.open_micro == 0
    loss = float(tr.window_loss) if c.N > 1 else float(loss)
    got = SimpleNamespace(modes=modes, inputs=inputs, loss=loss, finite=math.isfinite(loss), par=after.par, mo=after.mo, vo=after.vo, step=after.step,
                          skipped=after.skipped, lr=after.lr, bc1=after.bc1, bc2_sqrt=after.bc2_sqrt, grads=None)
    if got.finite:
        device_step(got, m, tr, c)
    return got


def device_step(got, m, tr, c):
    """The pre-clip gradient of a taken step and what the optimizer launch read: the raw gradient buffers (with grad_accum_steps > 1 SUMS over
    the window's scored tokens), their sum of squares as the device formed it, and the prescale 1 / count as the kernel forms it."""
    import numpy as np
    eng = m.llm_engine
    got.raw_grads = as_dict(m, c, eng.lora_g, m.conn_g if c.conn else None)
    got.sumsq, got.prescale = float(tr.sumsq), 1.0
    if c.N > 1:
        wg = tr.window_gradients()
        got.grads = as_dict(m, c, wg["lora_g"], wg["conn_g"])
        got.count = float(tr._window[1])
        got.prescale = float(np.float32(1.0) / np.float32(got.count))
    else:
        got.grads = got.raw_grads


@pytest.mark.parametrize("c", TC.CASES, ids=[c.name for c in TC.CASES])
def test_trainer_step_matrix(dev, c, tmp_path):
    oc, W = TC.pool()[:2]
    m, tr = build(c, tmp_path)
    sched = TC.schedule(c)
    ck = os.path.join(str(tmp_path), "ck.pt")
    worst, resumed_from, went_on, went_on_ref = 0.0, None, None, None
    for w, window in enumerate(sched):
        before = read_state(m, tr, c)
        assert before.open_micro == 0 and tr.skipped_steps == before.skipped
        hook = None
        if "resume" in c.event and w == 1 and c.N > 1:
            def hook():                                          # asked for mid-window: waits for the window to close
                tr._save_checkpoint(0, "ck.pt")
                assert tr._deferred_save is not None and not os.path.exists(ck)
        got = run_window(m, tr, c, window, w, hook)
        if "resume" in c.event and w == 1:
            if c.N == 1:
                tr._save_checkpoint(0, "ck.pt")
            assert os.path.exists(ck) and (c.N == 1 or tr._deferred_save is None)
        ref = RT.step(c, W, oc, before, [TC.host_batch(c, idx, bad) for idx, bad in window], w * c.N)
        ratio = TC.ratios(c, before, got, ref)
        print(f"{c.name} step {w} ({'finite' if ref.finite else 'NON-FINITE'}): {TC.show(ratio)}")
        worst = max(worst, TC.worst(ratio))
        assert TC.worst(ratio) <= 1.0, (c.name, w, ratio)
        if not ref.finite:
            assert tr.skipped_steps == before.skipped + 1 and got.step == before.step
        if "resume" in c.event and w == 2:
            went_on, resumed_from, went_on_ref = got, before, ref
    print(f"{c.name}: worst error / bar {worst:.3f}")
    # the launch forms the case promises
    f = TC.forms(c)
    assert any(isinstance(v, dict) for v in tr._graphs.values()) == (f["_replay"] or f["_replay_micro"])
    assert (c.N > 1 and isinstance(tr._close_graph, tuple)) == f["_close_graph"]
    assert tr.bwd_pieces == c.pieces and tr.train_connectors == bool(c.conn)
    # a validation batch is not augmented
    if c.audio_aug is not None or c.video_aug is not None:
        idx = sched[0][0][0]
        m.eval()
        a, v = tr._unpack(TC.trainer_batch(c, idx))[:2]
        m.train()
        want = RT.augmented_inputs(c, TC.host_batch(c, idx), RA.augment_seed(c.hyper.augment_seed, tr._augment_index(), 0), training=False)
        ratio = TC.input_ratios(c, [(a.float().cpu(), v.float().cpu())], [want[:2]])
        print(f"{c.name} validation batch: {TC.show(ratio)}")
        assert TC.worst(ratio) <= 1.0, ratio
    if "resume" in c.event:
        m2, tr2 = build(c, tmp_path / "resumed")
        tr2.load_checkpoint(ck)
        assert tr2._augment_index() == 2 * c.N and tr2.micro_step == 0
        state = read_state(m2, tr2, c)
        assert all(TC._same_bits(getattr(state, f)[k], getattr(resumed_from, f)[k]) for f in ("par", "mo", "vo") for k in state.par)
        assert (state.step, state.skipped) == (resumed_from.step, resumed_from.skipped) and tr2.skipped_steps == resumed_from.skipped
        again = run_window(m2, tr2, c, sched[2], 2)
        ratio = TC.ratios(c, resumed_from, again, went_on_ref)      # the resumed step against the restatement too: its schedule record, its update
        print(f"{c.name} step 2 resumed: {TC.show(ratio)}")
        assert TC.worst(ratio) <= 1.0, (c.name, "resumed", ratio)
        assert again.modes == went_on.modes
        assert all(TC._same_bits(x, y) for g, r in zip(again.inputs, went_on.inputs) for x, y in zip(g, r))
        rows = sum(RT.scored(TC.host_batch(c, idx)["labels"], oc.pad_token_id) for idx, _ in sched[2])      # one atomic add per scored row
        assert abs(again.loss - went_on.loss) <= Bar.atomic_sum_term(rows, max(abs(again.loss), abs(went_on.loss))), (again.loss, went_on.loss)
        assert all(TC._same_bits(getattr(again, f)[k], getattr(went_on, f)[k]) for f in ("par", "mo", "vo") for k in again.par)


# ---------------------------------------------------------------- two ranks
DDP_CASE = TC._case("two-ranks", "2", "eager", 1, "fp32", 0.05, "0.3/0.3", "dict", "spec", "off", 2, "one", "none")
DDP_WINDOW = {0: (TC.SIG["A"][0], TC.SIG["A"][1]), 1: (TC.SIG["A"][2], TC.SIG["A"][3])}


def _worker(rank, world, port, out_dir, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    c = DDP_CASE
    m, tr = build(c, os.path.join(out_dir, str(rank)), use_graph=False)
    assert tr.reducer.enabled and tr._rank == rank
    before = read_state(m, tr, c)
    modes, spans, same = [], [], []
    for j, idx in enumerate(DDP_WINDOW[rank]):
        unpacked = tr._unpack(TC.trainer_batch(c, idx))
        want = RT.augmented_inputs(c, TC.host_batch(c, idx), RA.augment_seed(c.hyper.augment_seed, j, rank))
        same.append(TC._same_bits(unpacked[0].cpu(), want[0]) and TC._same_bits(unpacked[1].cpu(), want[1]))
        spans.append(tr.audio_augment.last_spans.tolist())
        tr.train_step(*unpacked)
        modes.append(m.last_modality_modes.tolist())
    torch.cuda.synchronize()
    after = read_state(m, tr, c)
    wg = tr.window_gradients()
    to_np = lambda d: {k: v.numpy() for k, v in d.items()}      # noqa: E731
    q.put((rank, modes, spans, same, float(tr.window_loss), float(tr._window[1]), to_np(before.par), to_np(after.par), to_np(after.mo), to_np(after.vo),
           to_np(as_dict(m, c, wg["lora_g"], wg["conn_g"])), to_np(as_dict(m, c, m.llm_engine.lora_g, m.conn_g)),
           (after.step, after.skipped, after.lr, after.bc1, after.bc2_sqrt, float(tr.sumsq))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_window_against_the_restatement(dev, tmp_path):
    """N = 2 on 2 ranks with modality dropout, SpecAugment on features and training connectors: each rank draws the restatement's modes and
    masks for that rank, the ranks' draws differ, after one window the replicas hold the same bits, and they are the restatement's window over
    both ranks' micro-batches within the bars of the matrix."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 39700 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=300), q.get(timeout=300)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    c = DDP_CASE
    oc, W = TC.pool()[:2]
    t = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}      # noqa: E731
    r0, r1 = got
    assert all(r0[3]) and all(r1[3]), "a rank's augmented batch is not the restatement's for that rank"
    assert r0[1] != r1[1] and r0[2] != r1[2], "the two ranks drew the same modes or the same masks"
    assert r0[4] == r1[4] and r0[5] == r1[5]
    for i in (6, 7, 8, 9, 10, 11):                               # replicas: the same bits before and after, parameters, moments and gradients
        assert all((r0[i][k] == r1[i][k]).all() for k in r0[i]), i
    micro = [dict(TC.host_batch(c, idx), rank=r, micro=j) for r in (0, 1) for j, idx in enumerate(DDP_WINDOW[r])]
    before = SimpleNamespace(par=t(r0[6]), mo={k: torch.zeros_like(v) for k, v in t(r0[6]).items()}, vo={k: torch.zeros_like(v) for k, v in t(r0[6]).items()},
                             step=0, skipped=0)
    ref = RT.step(c, W, oc, before, micro, 0)
    import numpy as np
    step, skipped, lr, bc1, bc2s, sumsq = r0[12]
    have = SimpleNamespace(modes=r0[1] + r1[1], inputs=None, loss=r0[4], finite=math.isfinite(r0[4]), par=t(r0[7]), mo=t(r0[8]), vo=t(r0[9]),
                           grads=t(r0[10]), raw_grads=t(r0[11]), sumsq=sumsq, prescale=float(np.float32(1.0) / np.float32(r0[5])), step=step,
                           skipped=skipped, lr=lr, bc1=bc1, bc2_sqrt=bc2s)
    assert r0[5] == sum(ref.counts)
    ratio = TC.ratios(c, before, have, ref)
    print(f"two ranks: {TC.show(ratio)}")
    assert TC.worst(ratio) <= 1.0, ratio


# ---------------------------------------------------------------- the augmentation index after a skipped step
SKIP_CASE = TC._case("skipped-step", "1", "eager", 0, "fp32", 0.0, "off", "dict", "spec", "off", 1, "one", "none")


def test_augmentation_does_not_depend_on_the_log_interval(dev, tmp_path):
    """_train_epoch over [good, non-finite, good, good] with SpecAugment on, once looking at the losses after every batch and once never before
    the end: _sync_step() pulls global_step back to the device's count of steps TAKEN at every look, and the augmentation index must not move
    with it.  The augmented batches and the final parameters are equal bit for bit, the index counts all four batches, and a checkpoint
    carries it (a `_meta.json` without the entry falls back to global_step * grad_accum_steps)."""
    import json
    c = SKIP_CASE
    batches = [TC.trainer_batch(c, idx, bad) for idx, bad in zip(TC.SIG["A"][:4], (False, True, False, False))]
    runs = []
    for interval in (1, 100):
        m, tr = build(c, tmp_path / str(interval), train_dataloader=batches, log_interval=interval)
        seen, unpack = [], tr._unpack

        def recording(batch, seen=seen, unpack=unpack):
            out = unpack(batch)
            seen.append(out[0].clone())
            return out
        tr._unpack = recording
        tr._train_epoch(0)
        assert tr.skipped_steps == 1 and tr._sync_step() == 3 and tr._augment_index() == 4
        runs.append((m, tr, seen))
    (m1, t1, a1), (m2, t2, a2) = runs
    assert len(a1) == len(a2) == 4 and all(TC._same_bits(x.cpu(), y.cpu()) for x, y in zip(a1, a2))
    want = [RT.augmented_inputs(c, TC.host_batch(c, idx, bad), RA.augment_seed(c.hyper.augment_seed, i, 0))[0]
            for i, (idx, bad) in enumerate(zip(TC.SIG["A"][:4], (False, True, False, False)))]
    assert all(TC._same_bits(x.cpu(), y) for x, y in zip(a1, want))          # batch i draws with index i, skipped step or not
    assert torch.equal(m1.llm_engine.lora_p, m2.llm_engine.lora_p) and torch.equal(t1.m, t2.m) and torch.equal(t1.v, t2.v)
    t1._save_checkpoint(0, "ck.pt")
    ck = os.path.join(str(tmp_path / "1"), "ck.pt")
    meta = json.load(open(ck.replace(".pt", "_meta.json")))
    assert meta["augment_index"] == 4 and meta["global_step"] == 3
    m3, t3 = build(c, tmp_path / "resumed")
    t3.load_checkpoint(ck)
    assert t3.global_step == 3 and t3._augment_index() == 4
    del meta["augment_index"]
    json.dump(meta, open(ck.replace(".pt", "_meta.json"), "w"))
    t3.load_checkpoint(ck)
    assert t3._augment_index() == 3
