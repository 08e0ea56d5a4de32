"""The trainer-step case table and its host restatement, on the CPU (tests/trainer_cases.py, tests/refs64_trainer.py):
  * the list holds every pair of levels but the ones the code cannot take, and every path of forms() is seen taken and not taken;
  * the restatement is tied to what the suite already has: connector_step + the AdamW rule with every feature off, the reference-made
    optimizer fixture g5, refs64_modality's adjoint under mixed modes, and connector_step's defaults bit for bit;
  * every planted defect is caught by trainer_cases.ratios -- the comparison tests/test_trainer_matrix_gpu.py asserts with -- by more than 2 x
    its bar on every fp32 case that can carry it (the project's standing condition); the ratios on bf16 carriers are printed."""
import os

import numpy as np
import pytest
import torch

import bars as Bar
import connector_expect as CE
import refs64 as R
import refs64_augment as RA
import refs64_modality as RM
import refs64_trainer as RT
import trainer_cases as TC
from oracle import avsr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUNS = {}


def reference_run(c):
    """The restatement over the whole case, every step from the state the step before left: [(before, host micro-batches, aug index, result)]."""
    if c.name not in _RUNS:
        oc, W = TC.pool()[:2]
        before, out = TC.initial(c), []
        for w, window in enumerate(TC.schedule(c)):
            micro = [TC.host_batch(c, idx, bad) for idx, bad in window]
            res = RT.step(c, W, oc, before, micro, w * c.N)
            out.append((before, micro, w * c.N, res))
            before = res
        _RUNS[c.name] = out
    return _RUNS[c.name]


# ---------------------------------------------------------------- the list
def test_the_list_covers_its_pairs():
    assert TC.missing_pairs() == []
    assert len({c.name for c in TC.CASES}) == len(TC.CASES)
    for c in TC.CASES:                                           # no case holds a pair the code cannot take
        assert not [p for p in TC.IMPOSSIBLE if c.levels[p[0]] == p[1] and c.levels[p[2]] == p[3]], c.name
    # the two halves the trainer leaves out on a batch of tensors, at the lines IMPOSSIBLE names
    src = open(os.path.join(ROOT, "audio-visual-llm_amd", "avllm", "trainer.py")).read()
    assert "SpecAugment only (valid = all frames); noise needs raw waveforms" in src and "return aug.features(audio, None, " in src
    assert "flip and frame masks only (all frames counted); the crop needs raw frames" in src and "aug.pixels(video, None, " in src
    d = TC.BY_NAME["default-deployment"].levels
    assert d == dict(accum="1", launch="graph", conn=0, precision="bf16", drop=0.05, moddrop="off", form="dict", audio="off", video="off", pieces=1,
                     sigs="one", event="none")
    e = TC.BY_NAME["everything-on"].levels
    assert all(e[f] == FACTOR_ON[f] for f in TC.FACTORS if f != "precision")


FACTOR_ON = dict(accum="3f", launch="graph", conn=1, drop=0.05, moddrop="0.3/0.3", form="raw", audio="noise+spec", video="crop+flip+mask", pieces=2,
                 sigs="two", event="resume")


def test_every_form_is_seen_taken_and_not_taken():
    seen = {}
    for c in TC.CASES:
        for k, v in TC.forms(c).items():
            seen.setdefault(k, set()).add(bool(v))
    assert all(v == {True, False} for v in seen.values()), {k: v for k, v in seen.items() if v != {True, False}}


def test_schedules_reach_what_the_forms_promise():
    for c in TC.CASES:
        sched = TC.schedule(c)
        sizes = [len(w) for w in sched]
        assert sizes == {"1": [1] * 4, "2": [2] * 3, "3f": [3, 3, 2]}[c.accum], c.name
        visits = {}
        for w in sched:
            for idx, _ in w:
                visits[len(idx)] = visits.get(len(idx), 0) + 1
        assert (len(visits) == 2) == (c.sigs == "two") and visits[3] >= 3, (c.name, visits)      # signature A: warm, capture, replay
        assert len(sched) >= 3                                                                     # _close_graph: warm, capture, replay
        assert sum(bad for w in sched for _, bad in w) == (1 if "nonfinite" in c.event else 0)
        for w in sched:                                          # a mean of per-micro-batch means is not the window's token mean
            assert len(w) == 1 or len({RT.scored(TC.host_batch(c, idx)["labels"], 2) for idx, _ in w}) > 1, (c.name, w)
        # one width per signature: the prompt of a tokenised batch, the frames of a raw one
        assert len({(len(idx), TC.host_batch(c, idx)["prompt"].shape[1]) for w in sched for idx, _ in w}) == len(visits)


def test_a_poisoned_window_is_not_finite_whatever_the_modes():
    for c in TC.CASES:
        run = reference_run(c)
        assert [r.finite for *_, r in run] == [not any(bad for _, bad in w) for w in TC.schedule(c)], c.name
        for (before, _, _, r), w in zip(run, TC.schedule(c)):
            if not r.finite:
                assert (r.step, r.skipped) == (before.step, before.skipped + 1)
                assert all(torch.equal(r.par[k], before.par[k]) and torch.equal(r.mo[k], before.mo[k]) for k in before.par)
        assert all(TC.worst(TC.ratios(c, before, r, r)) == 0.0 for before, _, _, r in run), c.name      # the comparison of a step with itself


# ---------------------------------------------------------------- the restatement against existing anchors
def test_connector_step_defaults_are_todays_bits():
    """The function before it took modes= / dtype=, written out again, against the defaults; and modes of all zeros in fp32 against it."""
    oc, W, audio, video, labels, prompt, _ = TC.pool()
    idx = [0, 1, 2]
    a, v, lab, pr = audio[idx], video[idx], labels[idx], prompt[idx]
    Wc = dict(W)
    for name in ("audio_connector", "video_connector"):
        Wc[name] = {k: t.clone().requires_grad_(True) for k, t in W[name].items()}
    lora = {k: t.clone().requires_grad_(True) for k, t in W["lora"].items()}
    x, _, lb = O.prepare_llm_inputs(Wc, oc, a, v, pr, lab, training=True)
    x.retain_grad()
    loss = O.causal_lm_loss(O.llama_hidden(W["llama"], lora, oc.llama, oc.lora, x) @ W["llama"]["lm_head.weight"].T, lb)
    loss.backward()
    got = CE.connector_step(W, oc, a, v, pr, lab)
    assert torch.equal(got[0], loss.detach()) and torch.equal(got[1], x.grad)
    assert all(torch.equal(got[2][f"{n}.{k}"], t.grad) for n in ("audio_connector", "video_connector") for k, t in Wc[n].items())
    assert all(torch.equal(got[3][k], t.grad) for k, t in lora.items())
    both = CE.connector_step(W, oc, a, v, pr, lab, modes=[0, 0, 0])
    assert abs(float(both[0]) - float(loss.detach())) < Bar.F32_LOSS_ABS
    for k in CE.CONNECTOR_KEYS:
        assert float((both[2][k] - got[2][k]).abs().max()) <= Bar.F32_GRAD_REL_MAX * float(got[2][k].abs().max()), k


def test_all_features_off_is_connector_step_plus_adamw():
    """Three steps with every feature off against the loop of tests/test_connector_train_gpu.py::test_trainer_three_steps_vs_oracle (the oracle's
    own fp32 clip, AdamW and schedule), at that test's bars: loss 2e-4 per step, the update within 2e-2 of its own size."""
    c = TC._case("anchor", "1", "eager", 1, "fp32", 0.0, "off", "dict", "off", "off", 1, "one", "none")
    oc, W, audio, video, labels, prompt, _ = TC.pool()
    idx = [0, 1, 2]
    a, v, lab, pr = audio[idx], video[idx], labels[idx], prompt[idx]
    Wo = dict(W, lora={k: t.clone() for k, t in W["lora"].items()})
    for n in ("audio_connector", "video_connector"):
        Wo[n] = {k: t.clone() for k, t in W[n].items()}
    par = {"lora." + k: t for k, t in Wo["lora"].items()}
    par.update({f"{n}.{k}": t for n in ("audio_connector", "video_connector") for k, t in Wo[n].items()})
    keys = sorted(par)
    mo, vo = {k: torch.zeros_like(par[k]) for k in keys}, {k: torch.zeros_like(par[k]) for k in keys}
    state = TC.initial(c)
    init = {k: t.clone() for k, t in state.par.items()}
    for s in range(3):
        res = RT.step(c, W, oc, state, [TC.host_batch(c, idx)], s)
        ol, _, cg, lg = CE.connector_step(Wo, oc, a, v, pr, lab)
        assert abs(res.loss - float(ol)) < 2e-4, (s, res.loss, float(ol))
        g = {"lora." + k: t for k, t in lg.items()}
        g.update(cg)
        gl = [g[k] for k in keys]
        O.clip_grad_norm_(gl, c.hyper.grad_clip)
        for k, gk in zip(keys, gl):
            O.adamw_step(par[k], gk, mo[k], vo[k], s + 1, O.cosine_lr(c.hyper.lr, s, c.hyper.total_steps), wd=0.0 if k.endswith("bias") else c.hyper.weight_decay)
        state = res
    for group in (lambda k: k.startswith("lora."), lambda k: "connector" in k):
        num = sum(float(((state.par[k] - init[k]) - (par[k].double() - init[k])).pow(2).sum()) for k in filter(group, keys))
        den = sum(float((par[k].double() - init[k]).pow(2).sum()) for k in filter(group, keys))
        print(f"update error / update {(num / den) ** 0.5:.3e}")
        assert den > 0 and (num / den) ** 0.5 < 2e-2


def test_the_rule_reproduces_the_optimizer_fixture(golden_dir):
    """tests/golden/g5_optimizer.npz (torch.optim.AdamW + clip_grad_norm_ + CosineAnnealingLR as the reference wires them), at the bar of
    tests/test_oracle.py::test_optimizer_golden."""
    from types import SimpleNamespace
    g = np.load(f"{golden_dir}/g5_optimizer.npz")
    c = SimpleNamespace(conn=0, hyper=SimpleNamespace(lr=5e-5, total_steps=10, warmup_steps=0, grad_clip=0.5, weight_decay=0.01))
    zeros = lambda: {"lora.p": torch.zeros(1000, dtype=torch.float64)}      # noqa: E731
    s32 = s64 = SimpleNamespace(par={"lora.p": torch.from_numpy(g["p0"]).double()}, mo=zeros(), vo=zeros(), step=0, skipped=0)
    for s in range(3):
        assert abs(R.schedule(s + 1, 5e-5, 10)[0] - float(g[f"lr{s}"])) < 1e-12
        grad, want = {"lora.p": torch.from_numpy(g[f"g{s}"]).double()}, torch.from_numpy(g[f"p{s + 1}"]).double()
        # the fixture is fp32: the rule run in fp32 meets test_optimizer_golden's bar; run in float64 it stays within the fixture's own rounding,
        # three fp32 roundings of p per step taken (the decay product, the update term, the subtraction), 2^-24 relative each
        s32 = RT.apply_rule(c, s32, grad, True, dtype=torch.float32)
        s64 = RT.apply_rule(c, s64, grad, True)
        assert float((s32.par["lora.p"].double() - want).abs().max()) < 1e-7
        assert bool(((s64.par["lora.p"] - want).abs() <= (s + 1) * 3 * 2.0 ** -24 * want.abs()).all())
    assert s64.step == 3 and s64.skipped == 0


def test_mixed_modes_agree_with_the_adjoint_of_fuse_pool_rows():
    """The connector gradients of connector_step(modes=) are refs64_modality.fuse_pool_rows_bwd's rows of its own dx_embeds, pushed through the
    two linear layers: float64 against float64, so the two agree to rounding (1e-10 of the tensor's largest entry)."""
    oc, W, audio, video, labels, prompt, _ = TC.pool()
    idx = [0, 1, 2]
    a, v, lab, pr = audio[idx], video[idx], labels[idx], prompt[idx]
    modes = [RM.AUDIO, RM.VIDEO, RM.BOTH]
    loss, dx, cg, _ = CE.connector_step(W, oc, a, v, pr, lab, modes=modes, dtype=torch.float64)
    ha = O.whisper_encoder(W["whisper"], oc.whisper, a).double()
    hv = O.clip_vision_cls(W["clip"], oc.clip, v.reshape(-1, 3, 48, 48)).view(3, v.shape[1], -1).double()
    Ta, Tv = ha.shape[1], hv.shape[1]
    L = min(oc.max_seq_len, max(Ta, Tv))
    da, dv = RM.fuse_pool_rows_bwd(dx, modes, Ta, Tv, pr.shape[1], L, oc.fusion_scale)
    assert float(da[1].abs().max()) == 0.0 and float(dv[0].abs().max()) == 0.0 and float(da[0].abs().max()) > 0
    for name, d, h in (("audio_connector", da, ha), ("video_connector", dv, hv)):
        for k, want in ((".linear.weight", torch.einsum("btd,btk->dk", d, h)), (".linear.bias", d.sum((0, 1)))):
            assert float(want.abs().max()) > 0
            assert float((cg[name + k] - want).abs().max()) <= 1e-10 * float(want.abs().max()), name + k


def test_seeds_are_the_pinned_rules():
    assert RT.micro_seed(5, 1, 0, 2) == R.dropout_seed(5, 1, rank=2) == RM.step_seed(5, 2, 1)
    from test_grad_accum_host_cpu import micro_seed
    assert all(RT.micro_seed(s, k, m, r) == micro_seed(s, k, m, rank=r) for s in (1, 7) for k in (0, 2) for m in (0, 1, 5) for r in (0, 1))


# ---------------------------------------------------------------- planted defects
def carries(c, defect):
    """Whether case c can show the defect at all."""
    aug = c.audio != "off" or c.video != "off"
    return {"shared_aug_seed": c.N > 1 and aug, "modes_prev_seed": c.moddrop is not None, "modes_frozen": c.moddrop is not None,
            "dropped_stream_grad": c.moddrop is not None and bool(c.conn), "div_by_N": c.N > 1, "clip_per_micro": c.N > 1,
            "norm_lora_only": bool(c.conn), "shared_salt": c.audio != "off" and c.video != "off", "augment_validation": aug,
            "skip_advances_schedule": "nonfinite" in c.event, "decay_biases": bool(c.conn), "resume_from_zero": "resume" in c.event and aug,
            "lr_at_step_plus_skipped": "nonfinite" in c.event, "schedule_args_swapped": True}[defect]


def defect_ratio(c, defect):
    """The worst ratio over the case's steps, every step teacher-forced from the reference's state before it (a lower bound of it once a step
    exceeds 10)."""
    oc, W = TC.pool()[:2]
    worst = 0.0
    for before, micro, index, ref in reference_run(c):
        if defect == "augment_validation":                      # an eval-mode batch: only the inputs are compared
            seed = RA.augment_seed(c.hyper.augment_seed, index, 0)
            got, want = RT.augmented_inputs(c, micro[0], seed, False, {defect}), RT.augmented_inputs(c, micro[0], seed, False)
            worst = max(worst, TC.worst(TC.input_ratios(c, [got[:2]], [want[:2]])))
        else:
            worst = max(worst, TC.worst(TC.ratios(c, before, RT.step(c, W, oc, before, micro, index, wrong={defect}), ref)))
        if worst > 10.0:                                         # caught 5 x over: the later steps can only raise the figure
            break
    return worst


@pytest.mark.parametrize("defect", RT.DEFECTS)
def test_planted_defects_are_caught(defect):
    carriers = [c for c in TC.CASES if carries(c, defect)]
    fp32 = [c for c in carriers if c.precision == "fp32"]
    assert len(fp32) >= 2, "a planted defect needs fp32 cases that can carry it"
    got = {c.name: defect_ratio(c, defect) for c in carriers}
    print(f"{defect}: fp32 " + ", ".join(f"{c.name} {got[c.name]:.3g}" for c in fp32) + " | bf16 "
          + ", ".join(f"{c.name} {got[c.name]:.3g}" for c in carriers if c.precision != "fp32"))
    assert all(got[c.name] > 2.0 for c in fp32), {c.name: got[c.name] for c in fp32 if got[c.name] <= 2.0}
