"""ops.sample_rows(..., return_logprob=True) (csrc/sample.hip): the score of a draw is its log-probability under the distribution it was drawn
from, HF's transition score of a sampled token: float64 log_softmax of HF's own TemperatureLogitsWarper -> TopKLogitsWarper ->
TopPLogitsWarper chain on the same logits.  Bar 1e-4: the kept mass is an exact integer sum of exp(x - max) * 2^40 terms (each a float32
exponential, a few 1e-6 relative) and the rest is one subtraction and one logarithm in float32 on values below 32."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars  # noqa: E402
import refs64_select as R  # noqa: E402
from avllm import ops  # noqa: E402
from test_sample_gpu import kept, rows  # noqa: E402

TOL = 1e-4
CFGS = [(1.0, 0, 1.0), (0.7, 50, 0.9), (1.3, 0, 0.8), (1.0, 5, 1.0), (1.0, 1, 0.9)]
STEPS = 5


def draw_bar(row, t, k, p):
    """bars.select_logprob_bar of a row's kept distribution, capped at this file's earlier hand-set TOL."""
    keep, _ = R.kept(row, t, k, p)
    z = torch.as_tensor(R.scaled(row, t, k)[keep])
    ref = torch.log_softmax(z, 0)
    return min(TOL, bars.select_logprob_bar(ref, torch.log_softmax(z.float(), 0), int(keep.sum()), sizes=(z, z - z.max(), ref)))


def hf_chain(x, t, k, p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    h = x.clone()
    if t != 1.0:
        h = TemperatureLogitsWarper(t)(None, h)
    if k:
        h = TopKLogitsWarper(k)(None, h)
    if p < 1.0:
        h = TopPLogitsWarper(p)(None, h)
    return h


@pytest.mark.parametrize("V", [1000, 32000, 128256])
def test_logprob_of_the_draw_matches_hf_chain(dev, V):
    pytest.importorskip("transformers")
    B = 4
    x = rows(B, V, seed=V + 1)
    xd = x.to(dev)
    worst = 0.0
    for t, k, p in CFGS:
        h = hf_chain(x, t, k, p)
        want = torch.log_softmax(h.double(), dim=1)
        # continuous inputs: HF's kept set is the restatement's, so no draw should fall outside it
        for b in range(B):
            assert np.array_equal(kept(x[b].numpy(), t, k, p)[0], torch.isfinite(h[b]).numpy()), (V, t, k, p, b)
        bar = [draw_bar(x[b].numpy(), t, k, p) for b in range(B)]
        excluded = total = 0
        for step in range(STEPS):
            ids, lp = ops.sample_rows(xd, t, k, p, 11, step, return_logprob=True)
            assert torch.equal(ids, ops.sample_rows(xd, t, k, p, 11, step)), (V, t, k, p, step)
            ids, lp = ids.cpu(), lp.cpu()
            for b in range(B):
                w = float(want[b, ids[b]])
                total += 1
                if w == float("-inf"):                                  # a tie at the boundary that HF's chain does not keep
                    excluded += 1
                    continue
                d = abs(float(lp[b]) - w)
                worst = max(worst, d)
                assert d <= bar[b], (V, t, k, p, step, b, float(lp[b]), w, bar[b])
                assert float(lp[b]) <= 0.0
                if k == 1:
                    assert float(lp[b]) == 0.0
        assert excluded * 20 <= total, (V, t, k, p, excluded, total)
        assert excluded == 0, (V, t, k, p, excluded)                    # what the CPU check above predicts
    print(f"sample_rows logprob V={V}: max |d| against the HF chain {worst:.2e}")


def test_finished_rows_score_zero(dev):
    x = rows(4, 32000, seed=9).to(dev)
    unf = torch.tensor([True, False, True, False], device=dev)
    ids, lp = ops.sample_rows(x, 0.7, 50, 0.9, 3, 2, unfinished=unf.clone(), eos=5, pad=-7, return_logprob=True)
    free, lp_free = ops.sample_rows(x, 0.7, 50, 0.9, 3, 2, return_logprob=True)
    assert ids[1] == -7 and ids[3] == -7 and float(lp[1]) == 0.0 and float(lp[3]) == 0.0
    assert torch.equal(ids[[0, 2]], free[[0, 2]]) and torch.equal(lp[[0, 2]], lp_free[[0, 2]]) and (lp[[0, 2]] < 0).all()


def test_bf16_rows_and_infinite_maximum(dev):
    """bf16 logits are scored as their float32 values; a row whose maximum is +inf returns the argmax with score 0."""
    x = rows(4, 32000, seed=4, dtype=torch.bfloat16).to(dev)
    ids, lp = ops.sample_rows(x, 0.9, 40, 0.95, 1, 0, return_logprob=True)
    ids2, lp2 = ops.sample_rows(x.float(), 0.9, 40, 0.95, 1, 0, return_logprob=True)
    assert torch.equal(ids, ids2) and torch.equal(lp, lp2)
    y = x.float()
    y[2, 77] = float("inf")
    ids, lp = ops.sample_rows(y, 0.9, 40, 0.95, 1, 0, return_logprob=True)
    assert int(ids[2]) == 77 and float(lp[2]) == 0.0
