"""The float64 restatement of the smoothed objective (tests/refs64_loss.py) against torch autograd on the host: F.cross_entropy(label_smoothing=eps,
reduction="sum") over the shifted, scored rows + z * sum lse^2, value and gradient at 1e-12 relative; at (0, 0) it is refs64.cross_entropy."""
import pytest
import torch
import torch.nn.functional as F

import refs64 as R
import refs64_loss as RL

REL = 1e-12
CASES = [(0.0, 0.0), (0.1, 0.0), (0.0, 1e-2), (0.3, 1e-3)]


def autograd_loss(x64, labels, eps, z):
    """(sum over scored rows of the objective, the raw sums, d/dx) by torch's own cross entropy and autograd."""
    B, T, V = x64.shape
    x = x64.clone().requires_grad_(True)
    scored, tgt = RL.scored_rows(labels, V)
    rows, t = x[scored], tgt[scored]
    if rows.shape[0] == 0:
        return torch.zeros((), dtype=torch.float64), torch.zeros(3, dtype=torch.float64), torch.zeros_like(x64)
    lse = torch.logsumexp(rows, -1)
    total = F.cross_entropy(rows, t, label_smoothing=eps, reduction="sum") + z * (lse * lse).sum()
    total.backward()
    nll = F.cross_entropy(rows, t, reduction="sum").detach()
    u = (-F.log_softmax(rows, -1).mean(-1)).sum().detach()
    return total.detach(), torch.stack([nll, u, (lse * lse).sum().detach()]), x.grad


@pytest.mark.parametrize("eps,z", CASES)
@pytest.mark.parametrize("pat", RL.PATTERNS)
@pytest.mark.parametrize("scale", [1, 30])
@pytest.mark.parametrize("V", [8, 1001])
def test_restatement_is_torch_autograd(V, scale, pat, eps, z):
    B, T = 2, 40
    _, logits = RL.ce_logits(B, T, V, (V + 7) // 8 * 8, scale, torch.float32)
    labels = RL.ce_labels(pat, B, T, V)
    x64 = logits.double()
    gs = 0.37
    lse, loss_sum, count, terms, g = RL.smooth_cross_entropy(logits, labels, eps, z, grad_scale=gs)
    total, raw, grad = autograd_loss(x64, labels, eps, z)
    scored, _ = RL.scored_rows(labels, V)
    assert count == int(scored.sum())
    assert torch.equal(lse, torch.logsumexp(x64, -1).reshape(-1))
    assert abs(float(loss_sum) - float(total)) <= REL * max(abs(float(total)), 1e-300) or (count == 0 and float(loss_sum) == 0.0)
    for a, b in zip(terms.tolist(), raw.tolist()):
        assert abs(a - b) <= REL * max(abs(b), 1e-300) or (count == 0 and a == 0.0), (a, b)
    if count == 0:
        assert float(g.abs().max()) == 0.0
        return
    ref_g = grad * (gs / count)
    err = float((g - ref_g).abs().max())
    assert err <= REL * float(ref_g.abs().max()), (err, float(ref_g.abs().max()))
    assert float(g[~scored].abs().max()) == 0.0 if bool((~scored).any()) else True


@pytest.mark.parametrize("pat", RL.PATTERNS)
@pytest.mark.parametrize("V", [8, 1001])
def test_plain_case_is_refs64_cross_entropy(V, pat):
    B, T = 2, 40
    _, logits = RL.ce_logits(B, T, V, (V + 7) // 8 * 8, 30, torch.float32)
    labels = RL.ce_labels(pat, B, T, V)
    lse0, sum0, cnt0, g0 = R.cross_entropy(logits, labels, grad_scale=0.37)
    lse, loss_sum, count, terms, g = RL.smooth_cross_entropy(logits, labels, 0.0, 0.0, grad_scale=0.37)
    assert torch.equal(lse, lse0) and count == cnt0
    assert abs(float(loss_sum) - float(sum0)) <= REL * abs(float(sum0)) and abs(float(terms[0]) - float(sum0)) <= REL * abs(float(sum0))
    assert float((g - g0).abs().max()) <= REL * max(float(g0.abs().max()), 1e-300)
