"""CPU: the connector gradients rebuilt from the existing oracle functions (tests/connector_expect.py) equal the REFERENCE's own, recorded by
tools/make_golden_connector_grads.py in tests/golden/g11_connector_grads.npz (freeze_encoders=False on the g2 tiny model and batch).  Bar: the
one oracle/make_golden.py holds the oracle's LoRA gradients to, max |d| <= 5e-5 * max(1, max |g|).

On the g2 batch itself the reference's connector gradients are exactly zero (its scored labels sit in the first positions, which under causal
attention and the 544 -> 256 pooling see prompt rows only); case "b" is the same model and inputs with the labels cut to 24 columns, where
every connector tensor receives a gradient."""
import os

import numpy as np
import pytest
import torch

import connector_expect as CE
from oracle import weights as Wt


@pytest.fixture(scope="module")
def setup(golden_dir):
    z = np.load(os.path.join(golden_dir, "g11_connector_grads.npz"))
    cfg = Wt.tiny()
    W = Wt.all_weights(cfg, int(z["seed"]), lora_b_std=0.05)
    audio, video, labels, _ = Wt.synthetic_batch(cfg, 2, int(z["frames"]), seed=int(z["batch_seed"]))
    return z, cfg, W, audio, video, torch.from_numpy(z["prompt"]), labels


@pytest.mark.parametrize("case", ["", "b."])
def test_oracle_connector_grads_equal_the_reference(setup, case):
    z, cfg, W, audio, video, prompt, labels = setup
    lab = labels if case == "" else labels[:, :int(z["b.label_cols"])].contiguous()
    loss, dx, grads, _ = CE.connector_step(W, cfg, audio, video, prompt, lab)
    assert abs(float(loss) - float(z[case + "loss"])) <= 1e-5
    assert dx.shape == (2, lab.shape[1], cfg.llama.hidden) and float(dx.abs().max()) > 0
    for k in CE.CONNECTOR_KEYS:
        if case == "":          # the reference's gradient on the g2 batch is exactly zero: recorded as max |g|, compared as a zero tensor
            assert float(z["max_abs_grad." + k]) == 0.0
            ref = torch.zeros_like(grads[k])
        else:
            ref = torch.from_numpy(z[f"{case}grad.{k}"])
        d = float((grads[k] - ref).abs().max())
        print(f"{case or 'g2 '}{k}: max |g| {float(ref.abs().max()):.3e}  max |diff| {d:.3e}")
        assert d <= 5e-5 * max(1.0, float(ref.abs().max())), (k, d)
        if case == "b.":
            assert float(ref.abs().max()) > 1e-3          # a case on which the pin says something
