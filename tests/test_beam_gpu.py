"""Beam-search device ops (csrc/beam.hip): ops.beam_topk against torch.log_softmax + beam scores + torch.topk over num_beams*V, and
ops.kv_gather_rows against torch indexing, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402


def reference(logits, scores, nb, k):
    """The k + 1 best (score, beam, token) of HF's accumulated log-probabilities in float64 on the float32 inputs (the k + 1-th gives the gap
    at the boundary), and the float32 evaluation of the same entries (the yardstick of bars.select_logprob_bar)."""
    rows, V = logits.shape
    lp64 = torch.log_softmax(logits.double(), dim=-1)
    acc = (lp64 + scores.double()[:, None]).view(rows // nb, nb * V)
    s, i = torch.topk(acc, k=min(k + 1, nb * V), dim=1)
    acc32 = (torch.log_softmax(logits.float(), dim=-1) + scores[:, None]).view(rows // nb, nb * V).gather(1, i)
    lp = lp64.view(rows // nb, nb * V).gather(1, i)
    d = (logits.double() - logits.double().max(-1, keepdim=True).values).view(rows // nb, nb * V).gather(1, i)
    return s, (i // V).to(torch.int32), i % V, acc32, (d, lp)


def check(logits, scores, nb, k, tol=None):
    got_s, got_b, got_t = ops.beam_topk(logits, scores, nb, k)
    ref_s, ref_b, ref_t, cpu32, (d, lp) = reference(logits, scores, nb, k)
    if tol is None:
        # the derived bar of tests/bars.py where it is not larger than this file's earlier hand-set one (8 eps (max + 1) + 1e-6), else that one
        hand = 8 * torch.finfo(torch.float32).eps * (ref_s.abs().max().item() + 1.0) + 1e-6
        tol = min(hand, bars.select_logprob_bar(ref_s.cpu(), cpu32.cpu(), logits.shape[1], sizes=(d.cpu(), lp.cpu(), ref_s.cpu())))
    assert got_s.shape == (logits.shape[0] // nb, k)
    assert (got_s.double() - ref_s[:, :k]).abs().max().item() <= tol
    # a candidate's identity is pinned wherever its score is more than the rounding away from its neighbours'
    pad = torch.full_like(ref_s[:, :1], float("inf"))
    prev = torch.cat([pad, ref_s[:, :-1]], 1)[:, :k]
    nxt = torch.cat([ref_s[:, 1:], -pad], 1)[:, :k]
    clear = ((prev - ref_s[:, :k]) > 2 * tol) & ((ref_s[:, :k] - nxt) > 2 * tol)
    assert torch.equal(got_b[clear], ref_b[:, :k][clear]) and torch.equal(got_t[clear], ref_t[:, :k][clear])
    assert clear.float().mean() > 0.5
    return got_s, got_b, got_t


@pytest.mark.parametrize("V", [256, 32000, 32001, 128256])
@pytest.mark.parametrize("nb", [1, 2, 4, 5, 8, 16])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_beam_topk_grid(dev, B, nb, V):
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + nb * 10 + V)
    logits = torch.randn(B * nb, V, device="cuda", generator=g) * 4
    scores = -torch.rand(B * nb, device="cuda", generator=g) * 6
    check(logits, scores, nb, min(2 * nb, 32))


def test_beam_topk_strided_rows(dev):
    g = torch.Generator(device="cuda").manual_seed(3)
    big = torch.randn(8, 32000 + 77, device="cuda", generator=g) * 3
    logits = big[:, 5:5 + 32000]
    assert logits.stride(0) == 32077
    scores = -torch.rand(8, device="cuda", generator=g)
    check(logits, scores, 4, 8)
    for k in (1, 3, 32):
        check(logits, scores, 2, k)


def test_ties_go_to_the_lower_flat_index(dev):
    """Equal scores are ordered by j*V + v: planted equal logits within a row and across beams with equal beam scores."""
    V, nb = 1000, 4
    logits = torch.full((nb, V), -5.0, device="cuda")
    for j in range(nb):
        logits[j, [900, 17, 400]] = 3.0                    # three equal maxima per row, listed out of index order
        logits[j, 600] = 2.0
    scores = torch.zeros(nb, device="cuda")
    s, b, t = ops.beam_topk(logits, scores, nb, 16)
    want = [(j, v) for j in range(nb) for v in (17, 400, 900)] + [(j, 600) for j in range(nb)]
    assert [(int(x), int(y)) for x, y in zip(b[0], t[0])] == want
    assert torch.equal(s[0, :12], s[0, :1].expand(12)) and (s[0, 12:] < s[0, 11]).all()


def test_first_step_seed_scores(dev):
    """HF seeds beams 1..nb-1 with -1e9 at the first step (all rows equal); -inf beam scores never win over finite ones."""
    V, nb = 32000, 4
    g = torch.Generator(device="cuda").manual_seed(5)
    row = torch.randn(1, V, device="cuda", generator=g) * 3
    logits = row.expand(nb, V).contiguous()
    scores = torch.tensor([0.0, -1e9, -1e9, -1e9], device="cuda")
    s, b, t = ops.beam_topk(logits, scores, nb, 2 * nb)
    ref = torch.topk(torch.log_softmax(row[0], -1), 2 * nb)
    assert (b == 0).all() and torch.equal(t[0], ref.indices) and (s[0] - ref.values).abs().max() < 1e-5
    scores = torch.tensor([-float("inf"), -2.0, -float("inf"), -1e9], device="cuda")
    s, b, t = ops.beam_topk(logits, scores, nb, 2 * nb)
    assert (b == 1).all() and torch.equal(t[0], ref.indices)
    s, b, t = ops.beam_topk(logits, scores, nb, 32)
    assert (b[0, :32] == 1).all() and torch.isfinite(s).all()
    # -1e9 rows still order among themselves once the finite beams are exhausted: V = 3 gives 3 finite candidates of 8
    lg = torch.tensor([[1.0, 2.0, 3.0]] * 4, device="cuda")
    s, b, t = ops.beam_topk(lg, torch.tensor([0.0, -1e9, -1e9, -1e9], device="cuda"), 4, 8)
    assert b[0, :3].tolist() == [0, 0, 0] and t[0, :3].tolist() == [2, 1, 0]
    # -1e9 + log p rounds to -1e9 in fp32 (ulp 64): the rest are ties, in flat-index order
    assert (s[0, 3:] == -1e9).all() and b[0, 3:].tolist() == [1, 1, 1, 2, 2] and t[0, 3:].tolist() == [0, 1, 2, 0, 1]


def test_single_dominant_logit(dev):
    V, nb = 128256, 2
    logits = torch.zeros(nb, V, device="cuda")
    logits[0, 128255] = 1e4
    logits[1, 3] = 50.0
    s, b, t = ops.beam_topk(logits, torch.zeros(nb, device="cuda"), nb, 4)
    assert (b[0, 0], t[0, 0]) == (0, 128255) and s[0, 0].item() == 0.0
    assert (b[0, 1], t[0, 1]) == (1, 3) and abs(s[0, 1].item()) < 1e-4
    assert b[0, 2] == 1 and t[0, 2] == 0                     # then row 1's zeros (lowest index first), before row 0's (-1e4)


def test_beam_topk_bad_arguments(dev):
    logits = torch.zeros(34, 256, device="cuda")
    for nb, k in ((0, 2), (17, 4), (2, 0), (2, 33)):
        with pytest.raises(ValueError):
            ops.beam_topk(logits[: max(nb, 1) * 2], torch.zeros(max(nb, 1) * 2, device="cuda"), nb, k)
    lib = L.load()
    out_s = torch.empty(64, device="cuda"); out_b = torch.empty(64, device="cuda", dtype=torch.int32)
    out_t = torch.empty(64, device="cuda", dtype=torch.int64); ws = torch.empty(1 << 20, device="cuda", dtype=torch.uint8)
    sc = torch.zeros(34, device="cuda")
    for nb, k in ((17, 4), (2, 33), (0, 2), (2, 0)):        # the C entry rejects them too (AV_ERR_ARG = 1)
        rc = lib.avllm_beam_topk(L.ptr(logits), 256, 2, nb, 256, L.ptr(sc), k, L.ptr(out_s), L.ptr(out_b), L.ptr(out_t), L.ptr(ws),
                                 ws.numel(), L.stream_ptr())
        assert rc == 1, (nb, k, rc)


# ---------------------------------------------------------------- kv_gather_rows
MAPS = {
    "identity": lambda R: list(range(R)),
    "swap": lambda R: [r ^ 1 for r in range(R)],
    "cyclic": lambda R: [(r + 1) % R for r in range(R)],
    "all_from_one": lambda R: [R // 2] * R,
    "mixed": lambda R: [0, 0, 3, 2, 1, 5, 5, 6][:R] + [r for r in range(8, R)],
}


def caches(layers, rows, T, dkv, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(layers, rows, T, dkv, device="cuda", generator=g).to(dtype) for _ in range(2)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dkv", [4096, 1024, 136, 5])
@pytest.mark.parametrize("how", list(MAPS))
def test_gather_in_place(dev, dtype, dkv, how):
    layers, R, T, t0, t1 = 3, 8, 20, 5, 13
    k, v = caches(layers, R, T, dkv, dtype, dkv)
    parent = torch.tensor(MAPS[how](R), device="cuda", dtype=torch.int32)
    k0, v0 = k.clone(), v.clone()
    ops.kv_gather_rows(k, v, k, v, parent, t0, t1)
    for c, c0 in ((k, k0), (v, v0)):
        want = c0.clone()
        want[:, :, t0:t1] = c0[:, parent.long(), t0:t1]
        assert torch.equal(c, want)                          # outside [t0, t1) untouched: part of `want`


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("dkv", [4096, 1024])
def test_gather_out_of_place_broadcast(dev, dtype, dkv):
    """The prefix broadcast: a B-row cache into a B*nb-row cache with another T, parent[r] = r // nb; rows beyond [t0, t1) untouched."""
    layers, B, nb, S, T = 2, 3, 4, 9, 15
    ks, vs = caches(layers, B, S, dkv, dtype, 1)
    kd, vd = caches(layers, B * nb, T, dkv, dtype, 2)
    kd0, vd0 = kd.clone(), vd.clone()
    parent = (torch.arange(B * nb, device="cuda", dtype=torch.int32) // nb)
    ops.kv_gather_rows(ks, vs, kd, vd, parent, 0, S)
    for d, d0, s in ((kd, kd0, ks), (vd, vd0, vs)):
        assert torch.equal(d[:, :, :S], s[:, parent.long()]) and torch.equal(d[:, :, S:], d0[:, :, S:])
    ops.kv_gather_rows(ks, vs, kd, vd, parent.flip(0), 4, 4)               # t0 == t1: nothing moves
    assert torch.equal(kd[:, :, :S], ks[:, parent.long()])


def test_gather_many_rows_and_bad_arguments(dev):
    layers, R, T, dkv = 2, 40, 6, 1024
    k, v = caches(layers, R, T, dkv, torch.bfloat16, 9)
    parent = torch.randint(0, R, (R,), device="cuda", dtype=torch.int32)
    k0, v0 = k.clone(), v.clone()
    ops.kv_gather_rows(k, v, k, v, parent, 1, 6)
    assert torch.equal(k[:, :, 1:], k0[:, parent.long(), 1:]) and torch.equal(v[:, :, :1], v0[:, :, :1])
    with pytest.raises(ValueError):
        ops.kv_gather_rows(k, v, k, v, parent, 3, 7)
    with pytest.raises(ValueError):
        ops.kv_gather_rows(k, v, k, v, parent[:-1], 0, 1)
    with pytest.raises(ValueError):
        ops.kv_gather_rows(k, v, k, v, parent.long(), 0, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gather_at_the_row_limit(dev, dtype):
    """2048 destination rows: with the row count at the staging capacity every workgroup stages exactly one vector per row (all 2048 slots of its
    LDS buffer); 2049 rows must be refused and leave the caches as they were."""
    layers, T, dkv = 1, 2, 8
    for R_, ok in ((2048, True), (2049, False)):
        k, v = caches(layers, R_, T, dkv, dtype, R_)
        parent = torch.randint(0, R_, (R_,), device="cuda", dtype=torch.int32, generator=torch.Generator(device="cuda").manual_seed(R_))
        k0, v0 = k.clone(), v.clone()
        if ok:
            ops.kv_gather_rows(k, v, k, v, parent, 0, T)                            # in place, rows read and overwritten
            assert torch.equal(k, k0[:, parent.long()]) and torch.equal(v, v0[:, parent.long()])
            kd, vd = torch.zeros_like(k0), torch.zeros_like(v0)
            ops.kv_gather_rows(k0, v0, kd, vd, parent, 1, T)                        # out of place, one position
            assert torch.equal(kd[:, :, 1:], k0[:, parent.long(), 1:]) and torch.equal(vd[:, :, 1:], v0[:, parent.long(), 1:])
            assert not kd[:, :, :1].any() and not vd[:, :, :1].any()
        else:
            with pytest.raises(ValueError, match="2048"):
                ops.kv_gather_rows(k, v, k, v, parent, 0, T)
            assert torch.equal(k, k0) and torch.equal(v, v0)
