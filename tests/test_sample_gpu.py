"""ops.sample_rows (csrc/sample.hip): temperature -> top-k -> top-p -> one draw per row, against a NumPy restatement of HF's warper chain
(TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper with min_tokens_to_keep = 1) and this build's tie rule: in descending order the
kept set is the shortest prefix whose tail mass is <= 1 - top_p, plus every token whose scaled logit equals that of the last kept one.
Rows of <= 36,784 entries run from LDS, longer ones (128,256) from global memory; both are covered."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from avllm import ops  # noqa: E402
from refs64_select import draw_delta  # noqa: E402  (bars.draw_cdf_tol of a row: the derived slack of top-p membership)
from sample_ref import kept, kept_from_scaled, rows  # noqa: E402,F401  (the restatement lives there; importers of this file keep finding it here)

ALPHA = 1e-3            # significance level of the chi-square tests (fixed seeds: the outcome is deterministic)
P_SLACK = 1e-5          # top-p membership is checked against the kept set at top_p + the derived bars.draw_cdf_tol, capped at this (fp32 exp + fixed-point mass vs float64)


def draws(x, t, k, p, seeds, steps, row_seeds=None):
    out = [ops.sample_rows(x, t, k, p, s, st, row_seeds=row_seeds) for s in seeds for st in steps]
    return torch.stack(out).cpu().numpy()          # [len(seeds)*len(steps), B]


# --------------------------------------------------------------------------------------------- the restatement against HF
def test_restatement_matches_hf_warpers():
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    g = torch.Generator().manual_seed(0)
    for t, k, p in [(1.0, 50, 0.9), (0.7, 50, 0.9), (1.3, 0, 0.9), (1.0, 0, 0.5), (0.8, 200, 1.0), (1.0, 10, 0.3)]:
        s = torch.randn(4, 1000, generator=g, dtype=torch.float64) * 3
        h = s.clone()
        if t != 1.0:
            h = TemperatureLogitsWarper(t)(None, h)
        if k:
            h = TopKLogitsWarper(k)(None, h)
        if p < 1.0:
            h = TopPLogitsWarper(p)(None, h)
        for b in range(4):
            mine, _ = kept_from_scaled((s[b] / t).numpy(), k, p)
            assert np.array_equal(mine, torch.isfinite(h[b]).numpy()), (t, k, p, b)


# --------------------------------------------------------------------------------------------- 1. kept set
CFGS = [(0.7, 50, 0.9), (1.3, 0, 0.9), (1.0, 50, 1.0), (1.0, 2500, 0.95)]     # top-k + top-p (sorted survivors), top-p alone, top-k alone,
                                                                              # top-k past the sort capacity (radix top-p over the survivors)


@pytest.mark.parametrize("V", [1000, 32000, 128256])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sampled_ids_lie_in_kept_set(dev, V, dtype):
    B = 4
    x = rows(B, V, seed=V, dtype=dtype).to(dev)
    xf = x.float().cpu().numpy()
    for t, k, p in CFGS:
        ids = draws(x, t, k, p, seeds=range(6), steps=range(8))
        for b in range(B):
            keep, _ = kept(xf[b], t, k, min(1.0, p + min(P_SLACK, draw_delta(xf[b], t, k))) if p < 1 else p)
            bad = [i for i in ids[:, b] if not keep[i]]
            assert not bad, (V, dtype, t, k, p, b, bad[:5])


def test_strided_rows(dev):
    V = 32000
    wide = rows(3, V + 96, seed=5).to(dev)
    x = wide[:, :V]
    a = draws(x, 0.9, 50, 0.9, seeds=[3], steps=range(16))
    b = draws(x.contiguous(), 0.9, 50, 0.9, seeds=[3], steps=range(16))
    assert np.array_equal(a, b)


def tie_rows(V):
    """row 0: ties at the k-th value (k = 8: 5 tokens at 5.0, 10 at 4.0); row 1: a top-p boundary inside a tied group (1 at 3.0, 6 at 2.0,
    top_p 0.5 keeps all 7); row 2: 3000 tokens tied at the maximum (past the sort capacity, k = 50)."""
    g = np.random.RandomState(V)
    r = np.full((3, V), -8.0, np.float32)
    perm = g.permutation(V)
    r[0, perm[:5]] = 5.0
    r[0, perm[5:15]] = 4.0
    r[1, perm[:1]] = 3.0
    r[1, perm[1:7]] = 2.0
    r[2, perm[:3000]] = 1.0
    return r, [set(perm[:15].tolist()), set(perm[:7].tolist()), set(perm[:3000].tolist())]


@pytest.mark.parametrize("V", [32000, 128256])
def test_ties_are_kept_whole(dev, V):
    r, sets = tie_rows(V)
    for b, (k, p) in enumerate([(8, 1.0), (0, 0.5), (50, 0.9)]):
        for dtype in (torch.float32, torch.bfloat16):
            x = torch.from_numpy(r[b:b + 1]).to(dtype).to(dev)
            keep, prob = kept(x.float().cpu().numpy()[0], 1.0, k, p)
            assert set(np.nonzero(keep)[0].tolist()) == sets[b]
            ids = draws(x, 1.0, k, p, seeds=range(40), steps=range(20))[:, 0]
            assert set(ids.tolist()) <= sets[b], (V, b, dtype)
            # every member of the tied group is drawn (row 2: 800 draws over 3000 tokens: at least a fifth distinct)
            assert len(set(ids.tolist())) >= (min(len(sets[b]), 600) if b < 2 else 150), (b, len(set(ids.tolist())))


# --------------------------------------------------------------------------------------------- 2. distribution
def chi2_p(counts, probs, n):
    from scipy.stats import chi2
    e = probs * n
    big = e >= 5
    obs = np.append(counts[big], counts[~big].sum())
    exp = np.append(e[big], e[~big].sum())
    if exp[-1] < 5:
        obs[-2] += obs[-1]; exp[-2] += exp[-1]
        obs, exp = obs[:-1], exp[:-1]
    stat = ((obs - exp) ** 2 / exp).sum()
    return chi2.sf(stat, len(obs) - 1)


@pytest.mark.parametrize("V,t,k,p", [(32000, 1.0, 50, 0.9), (32000, 0.8, 0, 0.8), (128256, 1.2, 20, 1.0), (1000, 1.0, 0, 0.95)])
def test_distribution_chi_square(dev, V, t, k, p):
    B, steps = 8, 2500                                    # 20,000 draws: 8 rows (row seeds 0..7) x 2,500 steps
    base = np.full(V, -30.0, np.float32)
    g = np.random.RandomState(1)
    idx = g.choice(V, 60, replace=False)
    base[idx] = np.linspace(2.5, -1.5, 60).astype(np.float32) + g.uniform(-0.01, 0.01, 60).astype(np.float32)
    x = torch.from_numpy(np.tile(base, (B, 1))).to(dev)
    keep, prob = kept(base, t, k, p)
    assert 10 <= keep.sum() <= 60, keep.sum()
    ids = draws(x, t, k, p, seeds=[1234], steps=range(steps), row_seeds=torch.arange(B, dtype=torch.int32, device=dev)).ravel()
    assert keep[ids].all()
    counts = np.bincount(ids, minlength=V).astype(np.float64)
    sel = np.nonzero(keep)[0]
    pv = chi2_p(counts[sel], prob[sel], ids.size)
    assert pv > ALPHA, pv


# --------------------------------------------------------------------------------------------- 3. exact edges
@pytest.mark.parametrize("V", [1000, 32000, 128256])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_top_k_1_is_argmax(dev, V, dtype):
    x = rows(8, V, seed=3, dtype=dtype)
    x[1, 10] = x[1, 500] = x[1, V - 1] = 50.0                 # exact ties: lowest index wins
    x[2, :] = 0.0
    x[3, 7] = x[3, 3] = x[3].max() + 1
    x = x.to(dev)
    ref = ops.argmax_rows(x)
    for t, p, s in [(1.0, 1.0, 0), (0.3, 0.9, 1), (2.0, 0.2, 77)]:
        assert torch.equal(ops.sample_rows(x, t, 1, p, s, 5), ref)
    assert ref[1].item() == 10 and ref[2].item() == 0 and ref[3].item() == 3


@pytest.mark.parametrize("V", [1000, 128256])
def test_one_hot_row(dev, V):
    x = torch.full((3, V), float("-inf"), device=dev)
    x[0, 17] = 0.0
    x[1, V - 1] = 3.0
    x[2] = -1e4
    x[2, 999] = 0.0
    for t, k, p in [(1.0, 0, 1.0), (0.5, 50, 0.9), (1.0, 0, 0.3)]:
        ids = draws(x, t, k, p, seeds=range(4), steps=range(10))
        assert (ids[:, 0] == 17).all() and (ids[:, 1] == V - 1).all() and (ids[:, 2] == 999).all()


def test_whole_vocabulary_when_filters_off(dev):
    V = 32000
    x = (rows(8, V, seed=9, scale=1e-3)).to(dev)
    ids = draws(x, 1.0, 0, 1.0, seeds=[5], steps=range(200), row_seeds=torch.arange(8, dtype=torch.int32, device=dev)).ravel()
    assert len(set(ids.tolist())) > 1400              # 1,600 draws over 32,000 ids: ~1,560 distinct expected
    assert ids.min() < V // 20 and ids.max() > V - V // 20
    assert np.histogram(ids, bins=10, range=(0, V))[0].min() > 100


# --------------------------------------------------------------------------------------------- 4. determinism and independence
@pytest.mark.parametrize("V", [32000, 128256])
def test_repeats_bit_for_bit(dev, V):
    x = rows(8, V, seed=11).to(dev)
    for t, k, p in CFGS:
        a = draws(x, t, k, p, seeds=[7], steps=range(20))
        b = draws(x, t, k, p, seeds=[7], steps=range(20))
        assert np.array_equal(a, b)


@pytest.mark.parametrize("V", [32000, 128256])
def test_row_independent_of_neighbours(dev, V):
    x = rows(8, V, seed=12, scale=1.0).to(dev)
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4])
    for t, k, p in CFGS[:3]:
        for step in range(6):
            full = ops.sample_rows(x, t, k, p, 99, step)
            permuted = ops.sample_rows(x[perm.to(dev)].contiguous(), t, k, p, 99, step)
            assert torch.equal(permuted, full[perm.to(dev)])
            for r in (0, 3, 7):
                assert torch.equal(ops.sample_rows(x[r:r + 1], t, k, p, 99, step), full[r:r + 1])


def test_seeds_and_steps_change_the_stream(dev):
    x = rows(8, 32000, seed=13, scale=0.5).to(dev)
    a = draws(x, 1.0, 0, 0.95, seeds=[1], steps=range(32))
    b = draws(x, 1.0, 0, 0.95, seeds=[2], steps=range(32))
    assert (a != b).mean() > 0.9
    assert len(set(a[:, 0].tolist())) > 20                                  # steps differ
    rs = torch.arange(8, dtype=torch.int32, device=dev)
    same = torch.tile(x[:1], (8, 1)).contiguous()
    c = draws(same, 1.0, 0, 0.95, seeds=[1], steps=range(4), row_seeds=rs)
    assert all(len(set(r.tolist())) > 4 for r in c)                          # row seeds: identical rows draw independently


def test_step_from_device_and_mask(dev):
    x = rows(4, 32000, seed=14).to(dev)
    st = torch.tensor([6], dtype=torch.int32, device=dev)
    assert torch.equal(ops.sample_rows(x, 1.0, 50, 0.9, 3, st), ops.sample_rows(x, 1.0, 50, 0.9, 3, 6))
    free = ops.sample_rows(x, 1.0, 50, 0.9, 3, 6)
    unf = torch.tensor([True, False, True, True], device=dev)
    eos = int(free[2])
    got = ops.sample_rows(x, 1.0, 50, 0.9, 3, 6, unfinished=unf, eos=eos, pad=-7)
    assert got.tolist() == [free[0].item(), -7, eos, free[3].item()]
    assert unf.tolist() == [free[0].item() != eos, False, False, free[3].item() != eos]


# --------------------------------------------------------------------------------------------- 5. bad arguments
def test_bad_arguments(dev):
    x = rows(2, 1000, seed=1).to(dev)
    for t, k, p in [(0.0, 50, 0.9), (-1.0, 50, 0.9), (float("nan"), 50, 0.9), (1.0, 50, 0.0), (1.0, 50, 1.5), (1.0, 50, -0.1), (1.0, -1, 0.9)]:
        with pytest.raises(ValueError):
            ops.sample_rows(x, t, k, p, 0, 0)
