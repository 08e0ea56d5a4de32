"""label_smoothing / z_loss through ClipWhisperModel on the tiny golden model of tests/test_connector_train_gpu.py (make_model, Wt.tiny(), the g11
batch of 2 clips, dropout 0):
  * the training forward's "loss" and "nll_loss" against the float64 rule (tests/refs64_loss.py) evaluated on the logits the same forward
    returned -- the kernels' own input, so the comparison holds in fp32, bf16 and fp8 alike -- at the kernel test's loss_sum bar / count;
  * the eval() forward keeps the plain cross entropy, and reports what a model built without the keywords reports;
  * LoRA and connector gradients against host autograd through the oracle with only the loss swapped (tests/loss_expect.py), at the bars the
    plain-loss tests of this model use, with the (0, 0) run as the control in the same test, and the smoothed gradient at least a bar away
    from the plain one (the option is not silently dropped);
  * the default path: no loss_terms, and the bits of a model built without the keywords."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import connector_expect as CE  # noqa: E402
import loss_expect as LE  # noqa: E402
import refs64 as R  # noqa: E402
import refs64_loss as RL  # noqa: E402
from oracle import weights as Wt  # noqa: E402
from test_connector_train_gpu import make_model  # noqa: E402

EPS, Z = 0.1, 1e-3
COLS = 24                                                    # the pool branch of test_connector_train_gpu (32 + 512 rows -> 24)


@pytest.fixture(scope="module")
def batch(golden_dir):
    z = np.load(os.path.join(golden_dir, "g11_connector_grads.npz"))
    oc = copy.deepcopy(Wt.tiny())
    oc.max_seq_len = 512
    W = Wt.all_weights(oc, int(z["seed"]), lora_b_std=0.05)
    audio, video, labels, _ = Wt.synthetic_batch(oc, 2, int(z["frames"]), seed=int(z["batch_seed"]))
    return oc, W, audio, video, labels[:, :COLS].contiguous(), torch.from_numpy(z["prompt"])


_EXPECT = {}


def expectation(batch, eps, z):
    """The host's step under (eps, z), computed once and shared."""
    if (eps, z) not in _EXPECT:
        oc, W, audio, video, lab, prompt = batch
        _EXPECT[(eps, z)] = LE.smooth_step(W, oc, audio, video, prompt, lab, eps, z)
    return _EXPECT[(eps, z)]


def forward(m, batch, dev):
    _, _, audio, video, lab, prompt = batch
    return m(audio=audio.to(dev), video=video.to(dev), prompt=prompt.to(dev), labels=lab.to(dev))


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp8"])
def test_loss_is_the_rule_on_the_forwards_own_logits(dev, batch, precision):
    oc, W, _, _, lab, _ = batch
    kw = {"train_connectors": precision != "fp8"}
    m = make_model(oc, W, precision, label_smoothing=EPS, z_loss=Z, **kw)
    out = forward(m, batch, dev)
    labels = m._prep_labels(lab.to(dev))
    logits = out["logits"]
    _, ref_sum, cnt, ref_terms, _ = RL.smooth_cross_entropy(logits, labels, EPS, Z)
    term_bars, loss_bar = RL.sum_bars(logits, labels, EPS, Z)
    assert cnt > 0
    ref_loss, ref_nll = float(ref_sum) / cnt, float(ref_terms[0]) / cnt
    got_loss, got_nll = float(out["loss"].detach()), float(out["nll_loss"])
    # the quotient sum / count rounds once more
    print(f"{precision}: loss {got_loss:.6f} (rule {ref_loss:.6f}, bar {loss_bar / cnt:.2e}), nll {got_nll:.6f} (rule {ref_nll:.6f}, bar {term_bars[0] / cnt:.2e})")
    assert abs(got_loss - ref_loss) <= loss_bar / cnt + Bar.U32 * abs(ref_loss)
    assert abs(got_nll - ref_nll) <= term_bars[0] / cnt + Bar.U32 * abs(ref_nll)
    assert abs(ref_loss - ref_nll) > 10 * (loss_bar / cnt)                      # the two are not the same number at this (eps, z)
    # eval(): the plain cross entropy of the eval forward's logits, and what a model without the keywords reports
    m.eval()
    ev = forward(m, batch, dev)
    assert "nll_loss" not in ev
    S = ev["logits"].shape[1]
    lab_s = labels[:, :S] if labels.shape[1] > S else torch.cat([labels, labels.new_full((labels.shape[0], S - labels.shape[1]), -100)], 1)
    _, plain_sum, plain_cnt, _ = R.cross_entropy(ev["logits"], lab_s)
    _, plain_bar = RL.sum_bars(ev["logits"], lab_s, 0.0, 0.0)
    assert abs(float(ev["loss"]) - float(plain_sum) / plain_cnt) <= plain_bar / plain_cnt + Bar.U32 * float(plain_sum) / plain_cnt
    base = make_model(oc, W, precision, **kw).eval()
    ev0 = forward(base, batch, dev)
    assert torch.equal(ev0["logits"], ev["logits"])
    assert abs(float(ev0["loss"]) - float(ev["loss"])) <= Bar.atomic_sum_term(plain_cnt, float(ev["loss"]))


def lora_grads(m):
    return {k: v.float().cpu() for k, v in m.llm_engine.lora_views(m.lora_param.grad).items()}


def conn_grads(m):
    return {k: p.grad.detach().float().cpu() for k, p in m.named_parameters() if "connector" in k}


def judge(precision, what, got_loss, ref_loss, got, ref, keys):
    """The plain-loss tests' bars: fp32 per tensor at F32_GRAD_REL_MAX of its largest entry; bf16 the whole gradient at BF16_GRAD_REL_L2 and every
    tensor at BF16_GRAD_TENSOR_REL_L2.  -> the failures (empty: inside the bars)."""
    bad = []
    if precision == "fp32":
        if not abs(got_loss - ref_loss) < Bar.F32_LOSS_ABS:
            bad.append((what, "loss", got_loss, ref_loss))
        for k in keys:
            d, top = float((got[k] - ref[k]).abs().max()), float(ref[k].abs().max())
            print(f"{precision} {what} {k}: max |diff| {d:.3e}, max |ref| {top:.3e}")
            if not d <= Bar.F32_GRAD_REL_MAX * top:
                bad.append((what, k, d, top))
    else:
        if not abs(got_loss - ref_loss) < Bar.BF16_LOSS_ABS:
            bad.append((what, "loss", got_loss, ref_loss))
        whole = Bar.rel_l2(torch.cat([got[k].flatten() for k in keys]), torch.cat([ref[k].flatten() for k in keys]))
        print(f"{precision} {what}: whole gradient rel L2 {whole:.3e}")
        if not whole < Bar.BF16_GRAD_REL_L2:
            bad.append((what, "whole", whole))
        for k in keys:
            r = Bar.rel_l2(got[k], ref[k])
            if not r < Bar.BF16_GRAD_TENSOR_REL_L2:
                bad.append((what, k, r))
    return bad


@pytest.mark.parametrize("connectors", [False, True], ids=["lora", "lora+connectors"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_gradients_vs_host_autograd(dev, batch, precision, connectors):
    oc, W, *_ = batch
    runs = {}
    for eps, z in ((0.0, 0.0), (EPS, Z)):
        m = make_model(oc, W, precision, train_connectors=connectors, label_smoothing=eps, z_loss=z)
        out = forward(m, batch, dev)
        out["loss"].backward()
        ref_loss, ref_nll, ref_cg, ref_lg = expectation(batch, eps, z)
        got_l, got_c = lora_grads(m), conn_grads(m) if connectors else {}
        assert set(got_l) == set(ref_lg)
        bad = judge(precision, f"({eps}, {z}) lora", float(out["loss"].detach()), float(ref_loss), got_l, ref_lg, sorted(ref_lg))
        if connectors:
            bad += judge(precision, f"({eps}, {z}) connectors", float(out["loss"].detach()), float(ref_loss), got_c, ref_cg, list(CE.CONNECTOR_KEYS))
        if eps or z:
            nll_bar = Bar.F32_LOSS_ABS if precision == "fp32" else Bar.BF16_LOSS_ABS
            assert abs(float(out["nll_loss"]) - float(ref_nll)) < nll_bar
        runs[(eps, z)] = (bad, got_l, got_c)
    control, smoothed = runs[(0.0, 0.0)][0], runs[(EPS, Z)][0]
    assert not control, f"the plain-loss control is outside its bars: {control}"
    assert not smoothed, f"FINDING: the control is inside its bars, the smoothed case is not: {smoothed}"
    # the option reaches the gradient: smoothed and plain differ by more than the bar they are judged at
    for which, keys in ((1, sorted(runs[(EPS, Z)][1])), (2, list(CE.CONNECTOR_KEYS) if connectors else [])):
        if not keys:
            continue
        g1, g0 = runs[(EPS, Z)][which], runs[(0.0, 0.0)][which]
        if precision == "fp32":
            for k in keys:
                assert float((g1[k] - g0[k]).abs().max()) > Bar.F32_GRAD_REL_MAX * float(g0[k].abs().max()), k
        else:
            assert Bar.rel_l2(torch.cat([g1[k].flatten() for k in keys]), torch.cat([g0[k].flatten() for k in keys])) > Bar.BF16_GRAD_REL_L2


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_default_path_allocates_nothing_and_keeps_its_bits(dev, batch, precision):
    oc, W, *_ = batch
    res = []
    for kw in ({}, {"label_smoothing": 0.0, "z_loss": 0.0}):
        m = make_model(oc, W, precision, **kw)
        out = forward(m, batch, dev)
        out["loss"].backward()
        eng = m.llm_engine
        assert eng.loss_terms is None and eng.loss_opts is None and "nll_loss" not in out
        res.append((eng.lora_g.clone(), m.conn_g.clone(), out["logits"].clone()))
    assert float(res[0][0].abs().max()) > 0
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_constructor_refuses_values_out_of_range(dev, batch):
    oc, W, *_ = batch
    for kw, name in (({"label_smoothing": 1.0}, "label_smoothing=1.0"), ({"label_smoothing": -0.5}, "label_smoothing=-0.5"),
                     ({"label_smoothing": float("nan")}, "label_smoothing=nan"), ({"z_loss": -1.0}, "z_loss=-1.0"),
                     ({"z_loss": float("inf")}, "z_loss=inf"), ({"z_loss": "0.1"}, "z_loss")):
        with pytest.raises(ValueError, match=name):
            make_model(oc, W, "fp32", **kw)
