"""The token-selection kernels pinned to float64 at real vocabulary sizes: ops.sample_rows (csrc/sample.hip), ops.beam_topk (beam.hip),
ops.row_scores (token_score.hip) and the log-softmax stage of ops.logits_process (logits_process.hip), against the restatements of
tests/refs64_select.py under the derived bars of tests/bars.py ("token selection against float64"); tests/test_select_refs_cpu.py checks those
yardsticks on the host.  No bar comes from a kernel's output.

Every call goes through the C ABI the guarded way: logits are a column slice of a NaN-filled buffer (1e30-filled for sample_rows, which reads NaN as
-inf; row stride V + 5 for float32, which breaks the 16-byte alignment, V + 8 for bf16), outputs and beam_topk's workspace are views inside sentinel buffers whose borders must be intact
afterwards.  Each test prints "RATIO ..." with its worst error-to-bar ratio; the draw tests print "UNDECIDED ..." with their shares."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars  # noqa: E402
import refs64  # noqa: E402
import refs64_select as R  # noqa: E402
from avllm import lib as L  # noqa: E402
from sample_ref import rows as randn3  # noqa: E402
from test_token_score_gpu import VS as SCORE_VS, pattern_rows  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
NAN, NEG = float("nan"), float("-inf")
PAD = 64                                            # guard elements on either side of an output view
SENT = {torch.float32: 777.0, torch.int64: -777, torch.int32: -777, torch.uint8: 0xA5}


BIG = 1e30                                          # sample_rows reads NaN as -inf (no key, no mass), so NaN behind its rows would hide a read past V:
                                                    # its padding is a finite value that would take the whole mass and every argmax instead


def nan_slice(x, dtype=F32, pad=NAN):
    """x [rows, V] (host) as a column slice of a device buffer filled with `pad` (NaN) -> (view, row stride, buffer)."""
    rows, V = x.shape
    ld = V + (5 if dtype == F32 else 8)
    buf = torch.full((rows, ld), pad, device="cuda", dtype=dtype)
    buf[:, :V] = x.to(dtype)
    return buf[:, :V], ld, buf


def guarded(n, dtype):
    buf = torch.full((n + 2 * PAD,), SENT[dtype], device="cuda", dtype=dtype)
    return buf[PAD:PAD + n], buf


def intact(buf, n, what):
    s = SENT[buf.dtype]
    assert bool((buf[:PAD] == s).all()) and bool((buf[PAD + n:] == s).all()), f"{what}: the sentinel guard was written"


# ---------------------------------------------------------------- sample_rows
SAMPLE_VS, CFGS, STEPS, SEED, ROW_SEEDS = R.SAMPLE_VS, R.SAMPLE_CFGS, R.SAMPLE_STEPS, R.SAMPLE_SEED, R.SAMPLE_ROW_SEEDS


def sample_call(xs, ld, V, t, k, p, steps, row_seeds):
    """-> (ids [steps, rows], logprob [steps, rows]) on the host, drawn into guarded buffers."""
    rows = xs.shape[0]
    lib = L.load()
    ids, ids_buf = guarded(steps * rows, torch.int64)
    lp, lp_buf = guarded(steps * rows, F32)
    for st in range(steps):
        L.check(lib.avllm_sample_rows_scored(L.ptr(xs), ld, rows, V, float(t), int(k), float(p), SEED, L.ptr(row_seeds), st, None, None, -1, 0,
                                             L.ptr(ids[st * rows:]), L.ptr(lp[st * rows:]), L.dt_of(xs), L.stream_ptr()))
    torch.cuda.synchronize()
    intact(ids_buf, steps * rows, "sample_rows tokens")
    intact(lp_buf, steps * rows, "sample_rows logprob")
    return ids.view(steps, rows).cpu().numpy(), lp.view(steps, rows).cpu().numpy()


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("V", SAMPLE_VS)
def test_sample_rows_draws_and_logprob(dev, V, dtype):
    x = R.sample_input(V, dtype)
    xs, ld, _ = nan_slice(x, dtype, pad=BIG)
    xf = x.float().numpy()
    rs = torch.tensor(ROW_SEEDS, dtype=torch.int32, device="cuda")
    for t, k, p in CFGS:
        ids, lp = sample_call(xs, ld, V, t, k, p, STEPS, rs)
        und = plain = 0
        ratio = lp_ratio = 0.0
        for b in range(4):
            c = R.check_draws(xf[b], t, k, p, SEED, ROW_SEEDS[b], range(STEPS), ids[:, b])
            assert not c["errors"], (V, dtype, t, k, p, b, c["errors"][:3])
            und, plain, ratio = und + c["undecided"], plain + c["undecided_same_sets"], max(ratio, c["ratio"])
            lp_ratio = R.worst_of(lp_ratio, R.sample_logprob_ratio(xf[b], t, k, p, ids[:, b], lp[:, b]))
        n = 4 * STEPS
        print(f"UNDECIDED sample_rows V={V} {dtype} {(t, k, p)}: {und} of {n} (by the equal-sets rule alone: {plain})")
        print(f"RATIO sample_rows V={V} {dtype} {(t, k, p)}: u outside its interval / tol {ratio:.3f}, logprob {lp_ratio:.3f}")
        assert lp_ratio <= 1.0, (V, dtype, t, k, p, lp_ratio)
        assert und <= R.undecided_cap(V, k, n), (V, dtype, t, k, p, und)


def edge_rows(V, dtype):
    x = randn3(8, V, seed=3, dtype=dtype).float()
    x[1, 10] = x[1, V // 2] = x[1, V - 1] = 50.0                       # exact ties: the lowest index wins
    x[2, :] = 0.0                                                       # all equal
    x[3, 7] = x[3, 3] = x[3].max() + 1
    x[4, torch.arange(0, V, 3)] = NEG                                   # -inf entries
    x[5, :] = NEG                                                       # nothing but -inf
    x[6, torch.arange(1, V, 5)] = NAN                                   # NaN entries, the maximum among them
    x[6, int(x[6].nan_to_num(NEG).argmax())] = NAN
    x[6, 0] = NAN
    x[7, :] = NAN
    x[7, V - 2] = NEG                                                   # nothing but NaN and -inf
    return x.to(dtype).float()                                          # the values the kernel sees


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("V", SAMPLE_VS)
def test_top_k_1_is_the_documented_argmax(dev, V, dtype):
    """top_k = 1 = refs64.argmax_rows: the lowest index of the maximum, NaN read as -inf, whatever the temperature and top_p; score 0."""
    x = edge_rows(V, dtype)
    want = refs64.argmax_rows(x)
    xs, ld, _ = nan_slice(x, dtype, pad=BIG)
    for t, p in ((1.0, 1.0), (0.3, 0.9), (2.0, 0.2)):
        ids, lp = sample_call(xs, ld, V, t, 1, p, 2, None)
        assert ids[0].tolist() == want.tolist() == ids[1].tolist(), (V, dtype, t, p, ids[0].tolist(), want.tolist())
        assert (lp == 0.0).all()
    assert want[1] == 10 and want[2] == 0 and want[3] == 3 and want[5] == 0 and want[7] == 0


@pytest.mark.parametrize("V", [1000, 36785])
def test_nan_logits_are_never_drawn(dev, V):
    """NaN is read as -inf in every mode: the draws of a row with NaN entries are those of the row with -inf in their place."""
    x = randn3(2, V, seed=V + 2)
    x[:, torch.arange(2, V, 7)] = NAN
    x[0, int(x[0].nan_to_num(NEG).argmax())] = NAN
    xs, ld, _ = nan_slice(x, pad=BIG)
    clean, _, _ = nan_slice(x.nan_to_num(nan=NEG), pad=BIG)
    rs = torch.tensor(ROW_SEEDS[:2], dtype=torch.int32, device="cuda")
    for t, k, p in ((1.0, 0, 1.0), (0.7, 50, 0.9), (1.3, 2049, 0.95)):
        ids, lp = sample_call(xs, ld, V, t, k, p, 32, rs)
        ids2, lp2 = sample_call(clean, ld, V, t, k, p, 32, rs)
        assert np.array_equal(ids, ids2) and np.array_equal(lp, lp2), (V, t, k, p)
        for b in range(2):
            c = R.check_draws(x[b].numpy(), t, k, p, SEED, ROW_SEEDS[b], range(32), ids[:, b])
            assert not c["errors"], (V, t, k, p, b, c["errors"][:3])


# ---------------------------------------------------------------- beam_topk
BEAM_VS = [1, 3, 63, 4095, 4096, 4097, 8193, 32000, 131072, 131073, 151936]        # nseg * k crosses 1024 between 131,072 and 131,073 at k = 32
BEAM_NB = [1, 3, 14, 16]


def beam_call(xs, ld, B, nb, V, scores, k, logprobs=False):
    lib = L.load()
    need = lib.avllm_beam_topk_workspace_bytes(B * nb, V, k)
    ws, ws_buf = guarded(need, torch.uint8)
    s, s_buf = guarded(B * k, F32)
    b, b_buf = guarded(B * k, torch.int32)
    t, t_buf = guarded(B * k, torch.int64)
    fn = lib.avllm_beam_topk_logprobs if logprobs else lib.avllm_beam_topk
    L.check(fn(L.ptr(xs), ld, B, nb, V, L.ptr(scores), k, L.ptr(s), L.ptr(b), L.ptr(t), L.ptr(ws), need, L.stream_ptr()))
    torch.cuda.synchronize()
    for buf, n, what in ((ws_buf, need, "workspace"), (s_buf, B * k, "scores"), (b_buf, B * k, "beams"), (t_buf, B * k, "tokens")):
        intact(buf, n, f"beam_topk {what}")
    return s.view(B, k).cpu(), b.view(B, k).cpu().long(), t.view(B, k).cpu()


def ks_of(nb, V):
    return sorted({k for k in (1, 2 * nb, 32) if k <= nb * V})


def beam_normal(x, bs, B, nb, V, what):
    """One (x, beam scores) input in the normal mode at every k: the validity rule of refs64_select.beam_valid; returns the worst ratio."""
    s64 = R.beam_scores64(x, bs)
    ok = torch.isfinite(s64)
    cpu = torch.log_softmax(x, -1) + bs[:, None]
    lp64 = R.log_softmax64(x)
    d = x.double() - x.double().max(-1, keepdim=True).values
    bar = bars.select_logprob_bar(s64[ok], cpu[ok], V, sizes=(d[ok], lp64[ok], s64[ok]))
    xs, ld, _ = nan_slice(x)
    worst = 0.0
    for k in ks_of(nb, V):
        s, b, t = beam_call(xs, ld, B, nb, V, bs.cuda(), k)
        assert bool(((b >= 0) & (b < nb) & (t >= 0) & (t < V)).all()), (what, k)
        for i in range(B):
            good, r = R.beam_valid(s[i].numpy(), (b[i] * V + t[i]).numpy(), s64[i * nb:(i + 1) * nb].reshape(-1), k, bar)
            assert good, (what, k, i, r)
            worst = R.worst_of(worst, r)
    return worst


@pytest.mark.parametrize("V", BEAM_VS)
def test_beam_topk_against_float64(dev, V):
    B = 2
    worst = 0.0
    for nb in BEAM_NB:
        g = torch.Generator().manual_seed(V * 31 + nb)
        bs = -torch.rand(B * nb, generator=g) * 6
        fams = R.FAMILIES if V <= 8193 else ("randn", "banned")
        for fam in fams:
            x = R.family(fam, V, seed=V + nb, rows=B * nb)
            worst = R.worst_of(worst, beam_normal(x, bs, B, nb, V, (V, nb, fam)))
    print(f"RATIO beam_topk V={V}: worst |score - float64| / bar {worst:.3f}")


def beam_exact(lp, bs, B, nb, k, what):
    """logprobs=True on the exact family: scores bit for bit, identities equal to a stable host sort on (-score, flat index)."""
    V = lp.shape[1]
    xs, ld, _ = nan_slice(lp)
    s, b, t = beam_call(xs, ld, B, nb, V, bs.cuda(), k, logprobs=True)
    score = lp + bs[:, None]                                            # exact in float32 (test_select_refs_cpu checks the premise)
    for i in range(B):
        item = score[i * nb:(i + 1) * nb].reshape(-1)
        want = R.beam_order(item, k)
        got = (b[i] * V + t[i]).numpy()
        assert got.tolist() == want.tolist(), (what, k, i, got.tolist(), want.tolist())
        assert torch.equal(s[i].view(torch.int32), item[want].view(torch.int32)), (what, k, i)


@pytest.mark.parametrize("V", [3, 4095, 4096, 4097, 8193, 131073, 151936])
def test_beam_topk_exact_family(dev, V):
    B = 2
    for nb in BEAM_NB:
        lp = R.exact_logprobs(B * nb, V, seed=V + nb)
        lp[0, torch.arange(0, V, 2)] = NEG                              # banned entries
        bs = R.exact_beam_scores(B * nb, seed=V - nb)
        for k in ks_of(nb, V):
            beam_exact(lp, bs, B, nb, k, (V, nb))
    print(f"RATIO beam_topk exact V={V}: 0 (bit for bit)")


def test_beam_topk_planted_ties(dev):
    V, nb, B = 8193, 3, 2
    lp = R.exact_logprobs(B * nb, V, seed=9)
    lp[0, 4094:4098] = -0.25                                            # across the segment edge 4095 | 4096
    lp[0, [1023, 1024, 2047, 2048, 3071, 3072]] = -0.5                  # across the 1024-logit wave blocks of a segment
    lp[0, [4096 + 1023, 4096 + 1024, 8192]] = -0.5                      # and in the next segments
    lp[1] = lp[0]                                                       # across beams with equal beam scores
    lp[3, torch.linspace(0, V - 1, 40).long()] = 0.0                    # 40 equal maxima in one row, over all three segments
    lp[4] = NEG
    lp[4, [8192, 5, 4096]] = torch.tensor([-2.0, -2.0, -1.0])           # fewer than k finite entries
    lp[5] = NEG
    bs = torch.tensor([-1.0, -1.0, -1.5, 0.0, -0.125, -3.0])
    for k in (1, 6, 32):
        beam_exact(lp, bs, B, nb, k, "planted")
    # item 0 by the host sort: the ties across the segment edge, of both beams with their equal beam scores, in flat-index order
    want = R.beam_order((lp + bs[:, None])[:nb].reshape(-1), 8).tolist()
    assert want == [4094, 4095, 4096, 4097, V + 4094, V + 4095, V + 4096, V + 4097]
    # an item whose rows hold fewer than k finite entries in all: the rest comes back as -inf in flat-index order
    few = torch.full((2, 4097), NEG)
    few[0, [4096, 7]] = torch.tensor([-1.0, -1.0])
    few[1, 4095] = -0.5
    beam_exact(few, torch.tensor([-0.5, -1.0]), 1, 2, 8, "few")


def test_beam_topk_identical_rows_at_the_largest_vocabulary(dev):
    """The normal mode at V = 151,936 with identical rows and equal beam scores: equal maxima at 5, 4096 * 7 + 3 and 151,935 score the same bits in
    every beam and must come in flat-index order."""
    V, nb, B = 151936, 3, 2
    row = R.family("randn", V, seed=4)[0]
    at = [5, 4096 * 7 + 3, V - 1]
    row[at] = row.max() + 1.0
    x = row.expand(B * nb, V).contiguous()
    bs = torch.tensor([-1.0, -1.0, -1.0, -2.0, -2.0, -2.0])
    worst = beam_normal(x, bs, B, nb, V, "identical rows")
    xs, ld, _ = nan_slice(x)
    for k in (9, 32):
        s, b, t = beam_call(xs, ld, B, nb, V, bs.cuda(), k)
        for i in range(B):
            assert (b[i, :9] * V + t[i, :9]).tolist() == [j * V + v for j in range(nb) for v in at], (k, i)
            assert bool((s[i, :9] == s[i, 0]).all()) and bool((s[i, 9:] < s[i, 8]).all())
    print(f"RATIO beam_topk identical rows V={V}: {worst:.3f}")


# ---------------------------------------------------------------- row_scores
@pytest.mark.parametrize("temperature", [1.0, 0.7, 2.5])
@pytest.mark.parametrize("V", SCORE_VS)
def test_row_scores_against_float64(dev, V, temperature):
    x, tok = pattern_rows(V, seed=V)
    P = x.shape[0]
    want_lp, want_ent = R.row_scores64(x, tok, temperature)
    cpu_lp, cpu_ent = R.row_scores64(x, tok, temperature, dtype=F32)
    xs, ld, _ = nan_slice(x)
    lib = L.load()
    lp, lp_buf = guarded(P, F32)
    ent, ent_buf = guarded(P, F32)
    tok_d = tok.cuda()
    L.check(lib.avllm_row_scores(L.ptr(xs), ld, P, V, L.ptr(tok_d), float(temperature), L.ptr(lp), L.ptr(ent), L.F32, L.stream_ptr()))
    torch.cuda.synchronize()
    intact(lp_buf, P, "row_scores logprob")
    intact(ent_buf, P, "row_scores entropy")
    lp, ent = lp.cpu(), ent.cpu()
    y = (x / torch.tensor(temperature)).double()
    r_lp = r_ent = 0.0
    for r in range(P):
        fin = y[r][torch.isfinite(y[r])]
        if torch.isinf(want_lp[r]):
            assert float(lp[r]) == float(want_lp[r]), (V, temperature, r)
        else:
            bar = bars.select_logprob_bar(want_lp[r:r + 1], cpu_lp[r:r + 1], V, sizes=(fin, fin - fin.max(), want_lp[r]))
            r_lp = R.worst_of(r_lp, R.ratio(float(lp[r]) - float(want_lp[r]), bar))
        bar = bars.select_entropy_bar(y[r:r + 1], want_ent[r:r + 1], cpu_ent[r:r + 1])
        r_ent = R.worst_of(r_ent, R.ratio(float(ent[r]) - float(want_ent[r]), bar))
    print(f"RATIO row_scores V={V} t={temperature}: logprob {r_lp:.3f}, entropy {r_ent:.3f}")
    assert r_lp <= 1.0 and r_ent <= 1.0, (V, temperature, r_lp, r_ent)


# ---------------------------------------------------------------- the log-softmax stage of logits_process
@pytest.mark.parametrize("V", [97, 4097, 128256, 151936])
def test_log_softmax_stage_against_float64(dev, V):
    x = torch.cat([R.family(fam, V, seed=V + 3) for fam in R.FAMILIES])
    rows = x.shape[0]
    ref = R.log_softmax64(x)
    cpu = torch.log_softmax(x, -1)
    d = x.double() - x.double().max(-1, keepdim=True).values
    lib = L.load()
    outs = []
    for _ in range(2):
        xs, ld, buf = nan_slice(x)
        L.check(lib.avllm_logits_process(L.ptr(xs), ld, rows, V, None, 0, None, 0, None, 1.0, 0, 0, -1, 1, L.F32, L.stream_ptr()))
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:, V:]).all()), "logits_process wrote past the row"
        outs.append(xs.cpu())
    got = outs[0]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))           # repeats bit for bit
    worst = 0.0
    for r in range(rows):
        ok = torch.isfinite(ref[r])
        assert torch.equal(torch.isinf(got[r]), ~ok) and bool((got[r][~ok] == NEG).all())
        bar = bars.select_logprob_bar(ref[r][ok], cpu[r][ok], V, sizes=(d[r][ok], ref[r][ok]))
        worst = R.worst_of(worst, R.ratio((got[r].double() - ref[r])[ok], bar))
    print(f"RATIO logits_process log_softmax V={V}: {worst:.3f}")
    assert worst <= 1.0, (V, worst)
