"""CPU: the restatements of tests/refs64_modality.py pinned down -- the adjoint to torch autograd through the forward, the draw rule of
avllm_modality_draw to its edge cases, to binomial frequencies and to the three mode vectors the graph test relies on -- and the argument
rules of the constructor and of modality_mask that need no device."""
import math

import pytest
import torch

import refs64_modality as RM
from test_connector_kernels_gpu import GEOMS

TWO_INPUT = [g for g in GEOMS if g[0] and g[1]]


@pytest.mark.parametrize("Ta,Tv,P,L,S", TWO_INPUT)
def test_adjoint_restatement_is_autograd_of_forward(Ta, Tv, P, L, S):
    B, D, fs, modes = 4, 5, 0.3, [0, 1, 2, 0]
    g = torch.Generator().manual_seed(S + 10 * Ta)
    a = torch.randn(B, Ta, D, generator=g, dtype=torch.float64, requires_grad=True)
    v = torch.randn(B, Tv, D, generator=g, dtype=torch.float64, requires_grad=True)
    pe = torch.randn(B, P, D, generator=g, dtype=torch.float64) if P else None
    dx = torch.randn(B, S, D, generator=g, dtype=torch.float64)
    out = RM.fuse_pool_rows(a, v, pe, modes, L, S, fs)
    assert out.shape == (B, S, D)
    out.backward(dx)
    da, dv = RM.fuse_pool_rows_bwd(dx, modes, Ta, Tv, P, L, fs)
    assert float((da - a.grad).abs().max()) <= 1e-14 and float((dv - v.grad).abs().max()) <= 1e-14
    assert float(dv[1].abs().max()) == 0.0 and float(da[2].abs().max()) == 0.0           # the unused stream
    assert float(da[1].abs().max()) > 0.0 and float(dv[2].abs().max()) > 0.0
    if Ta > L:
        assert float(da[:, L:].abs().max()) == 0.0


def test_forward_restatement_modes():
    """Uniform modes are the one-input rule (the other alone, scale 1); the unused stream is never touched."""
    B, Ta, Tv, P, L, S, D, fs = 3, 9, 7, 3, 9, 5, 4, 0.3
    g = torch.Generator().manual_seed(0)
    a, v, pe = torch.randn(B, Ta, D, generator=g), torch.randn(B, Tv, D, generator=g), torch.randn(B, P, D, generator=g)
    nan_a, nan_v = a.clone(), v.clone()
    nan_a[2], nan_v[1] = float("nan"), float("nan")
    clean = RM.fuse_pool_rows(a, v, pe, [0, 1, 2], L, S, fs)
    assert torch.equal(RM.fuse_pool_rows(nan_a, nan_v, pe, [0, 1, 2], L, S, fs), clean)
    zeros = torch.zeros_like
    only_a = RM.fuse_pool_rows(a, zeros(v), pe, [1] * B, L, S, fs)
    assert torch.equal(only_a[1], clean[1])
    one = RM.fuse_pool_rows(a, zeros(v), pe, [0] * B, L, S, 1.0)                         # fs = 1: a alone through the two-input rule
    assert float((one - only_a).abs().max()) <= 1e-15


def test_draw_edge_cases():
    for seed in (0, 7, 0xFFFFFFFF):
        assert RM.draw(257, 0.0, 0.0, seed) == [0] * 257
        assert RM.draw(257, 1.0, 0.0, seed) == [2] * 257
        assert RM.draw(257, 0.0, 1.0, seed) == [1] * 257
        assert 0 not in RM.draw(4096, 0.5, 0.5, seed)
        given = [(b % 4) for b in range(64)]                                             # 3 is not a mode: drawn like 0
        out = RM.draw(64, 0.5, 0.5, seed, mode_in=given)
        assert all(o == gv for o, gv in zip(out, given) if gv in (1, 2))
        assert out == [gv if gv in (1, 2) else d for gv, d in zip(given, RM.draw(64, 0.5, 0.5, seed))]
    assert RM.threshold(0.0) == 0 and RM.threshold(1.0) == 1 << 24 and RM.threshold(0.5) == 1 << 23
    assert RM.av_pair_hash(5, 9) == RM.av_hash32(9 ^ RM.av_hash32(5))


@pytest.mark.parametrize("pa,pv", [(0.25, 0.25), (0.1, 0.4), (0.05, 0.0)])
@pytest.mark.parametrize("seed", [0, 1, 12345, 0xDEADBEEF, RM.step_seed(1)])
def test_draw_frequencies(seed, pa, pv):
    """Each dropped mode within 5 standard deviations of a binomial over 65,536 rows."""
    N = 65536
    modes = RM.draw(N, pa, pv, seed)
    for p, k, nm in ((pa, RM.VIDEO, "audio dropped"), (pv, RM.AUDIO, "video dropped")):
        f = modes.count(k) / N
        if p == 0.0:
            assert f == 0.0
            continue
        sigma = math.sqrt(p * (1 - p) / N)
        print(f"seed {seed:#x} p=({pa}, {pv}) {nm}: frequency {f:.5f}, {abs(f - p) / sigma:.2f} sigma")
        assert abs(f - p) <= 5 * sigma, (nm, f, p)


def test_draw_of_the_first_three_trainer_steps():
    """What tests/test_modality_trainer_gpu.py relies on: three different mode vectors on a 2-clip batch at (0.3, 0.3)."""
    assert RM.step_seed(1) == (0x9E3779B1 + 12345) & 0xFFFFFFFF
    assert [tuple(RM.draw(2, 0.3, 0.3, RM.step_seed(s))) for s in (1, 2, 3)] == [(2, 0), (0, 2), (0, 0)]


# ---------------------------------------------------------------- argument rules
def test_constructor_refuses_bad_probabilities():
    from avllm.model import ClipWhisperModel
    for kw, who in (({"modality_dropout_audio": -0.1}, "modality_dropout_audio"), ({"modality_dropout_video": 1.5}, "modality_dropout_video"),
                    ({"modality_dropout_audio": "0.3"}, "modality_dropout_audio"),
                    ({"modality_dropout_audio": 0.6, "modality_dropout_video": 0.6}, "modality_dropout_audio \\+ modality_dropout_video"),
                    ({"modality_dropout_video": 0.2, "modality": "audio"}, "modality_dropout_video"),
                    ({"modality_dropout_audio": 0.2, "modality": "video"}, "modality_dropout_audio")):
        with pytest.raises(ValueError, match=who):
            ClipWhisperModel(**kw)


def test_mask_parsing():
    from avllm.model import parse_modality_mask
    assert parse_modality_mask([0, 1, 2], 3).tolist() == [0, 1, 2]
    assert parse_modality_mask(("both", "audio", "video"), 3).tolist() == [0, 1, 2]
    t = parse_modality_mask(torch.tensor([2, 0], dtype=torch.int64), 2)
    assert t.dtype == torch.int32 and t.tolist() == [2, 0]
    for bad, B, msg in (([0, 1], 3, "2 entries for a batch of 3"), ([0, 3], 2, r"modality_mask\[1\]"), (["both", "lips"], 2, r"modality_mask\[1\]"),
                        ([0, -1], 2, r"modality_mask\[1\]"), ([0.0, 1.0], 2, r"modality_mask\[0\]"), ([True, False], 2, r"modality_mask\[0\]"),
                        (torch.tensor([0.0, 1.0]), 2, "integer tensor"), (torch.zeros(2, 2, dtype=torch.int32), 2, "1-d"), (1, 1, "list or a tensor")):
        with pytest.raises(ValueError, match=msg):
            parse_modality_mask(bad, B)
