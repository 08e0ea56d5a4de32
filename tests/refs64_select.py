"""float64 restatements of the token-selection kernels (csrc/sample.hip, beam.hip, token_score.hip, the log-softmax stage of logits_process.hip)
on the float32 values the kernels see (the division by the float32 temperature is done in float32, as on the device), a host emulation of
each kernel's documented arithmetic in float32, and the input families.  The bars that go with them are in bars.py ("token selection against
float64"); tests/test_select_refs_cpu.py holds the emulations to those bars and shows that planted faults exceed them.

NaN logits follow argmax_kernel's rule in sample_rows: they are read as -inf (never kept, never drawn).  beam_topk leaves NaN to the caller."""
import numpy as np
import torch

from generate_ref import h32
from sample_ref import kept_from_scaled, rows

F64 = torch.float64
NEG = float("-inf")
SEG = 4096                      # beam.hip: logits per segment
TILE = 256                      # sample.hip: entries per draw tile
FAMILIES = ("randn", "dominant", "flat", "banned", "pm80")


# ---------------------------------------------------------------- NaN-proof comparisons
def ratio(err, bar):
    """max |err| / bar as a float, refusing NaN and inf: a NaN result (what a read past V into the NaN padding gives) compares False with every
    bound and Python's max(0.0, nan) is 0.0, so a plain `max(worst, err / bar)` followed by `<= 1` would let it through."""
    e = torch.as_tensor(err, dtype=torch.float64).abs().reshape(-1)
    assert bool(torch.isfinite(e).all()), "a result that is NaN or infinite where the reference is finite"
    assert bar == bar and bar >= 0.0, f"bar {bar}"
    m = float(e.max()) if e.numel() else 0.0
    return m / bar if bar > 0 else (0.0 if m == 0.0 else float("inf"))


def worst_of(worst, r):
    """max(worst, r) that fails on a NaN instead of dropping it."""
    r = float(r)
    assert r == r, "a NaN ratio"
    return max(worst, r)


# ---------------------------------------------------------------- families
def family(name, V, seed, rows=1):
    """float32 rows [rows, V] of one input family."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, V, generator=g) * 4
    if name == "randn":
        return x
    if name == "dominant":                                               # one logit 60 above the rest
        j = torch.randint(0, V, (rows,), generator=g)
        x[torch.arange(rows), j] = x.max(1).values + 60.0
        return x
    if name == "flat":
        return torch.full((rows, V), 1.5)
    if name == "banned":                                                 # a scattered half at -inf (never the whole row)
        ban = torch.rand(rows, V, generator=g) < 0.5
        ban[:, int(torch.randint(0, V, (1,), generator=g))] = False
        return x.masked_fill(ban, NEG)
    if name == "pm80":                                                   # +-80: the max subtraction matters
        return x * 0.25 + torch.where(torch.rand(rows, V, generator=g) < 0.5, 80.0, -80.0)
    raise ValueError(name)


def exact_logprobs(rows, V, seed, lo=-16.0, hi=-1.0):
    """The `exact` family of beam_topk(logprobs=True): multiples of 2^-3 in [lo, hi] (a subrange of [-16, 0])."""
    g = torch.Generator().manual_seed(seed)
    n = int(round((hi - lo) * 8)) + 1
    return lo + torch.randint(0, n, (rows, V), generator=g).float() / 8.0


def exact_beam_scores(rows, seed):
    g = torch.Generator().manual_seed(seed)
    return -torch.randint(0, 129, (rows,), generator=g).float() / 8.0


# ---------------------------------------------------------------- sample_rows
# The draw cases of tests/test_select_pin_gpu.py, stated here so that tests/test_select_refs_cpu.py runs the float64 reference alone over the very
# same rows.  36,784 is the last row length sample.hip holds in LDS, 36,785 the first it re-reads; k = 64 | 65: a sort of 64 | 128 slots;
# 2048 | 2049: the last sorted | the first radix top-p.
SAMPLE_VS = [1000, 36784, 36785, 128256, 151936]
SAMPLE_CFGS = [(0.7, 50, 0.9), (1.0, 64, 0.9), (1.0, 65, 0.9), (1.3, 2048, 0.95), (1.3, 2049, 0.95), (1.0, 0, 0.95), (1.0, 0, 1.0), (1.0, 50, 1.0)]
SAMPLE_STEPS, SAMPLE_SEED, SAMPLE_ROW_SEEDS = 64, 1234, [5, 11, 2, 7]


def sample_input(V, dtype):
    """randn * 3 rows [4, V].  The generator seed is V + 1: whether a draw is decided depends on the reference alone (u and the float64 CDF, never
    the token a kernel returns), and with seed V one row at V = 36,784 has its top-p boundary within delta of a token of mass 1e-4 under
    k = 2049, which leaves 21 of its draws open to either kept set: more than the cap of a twentieth, for any kernel."""
    return rows(4, V, seed=V + 1, dtype=dtype)


def undecided_cap(V, k, n):
    """At most a fifth of n draws undecided where top-k is off, a twentieth where it is on."""
    return n // (20 if 0 < k < V else 5)


def scaled(row, t, k=0):
    """One row as sample.hip scales it: float32 division (t = 1 when top_k == 1), NaN read as -inf, then float64."""
    r = np.asarray(row, np.float32)
    y = (r / np.float32(1.0 if k == 1 else t)).astype(np.float64)
    return np.where(np.isnan(y), -np.inf, y)


def _p32(p):
    return float(np.float32(p))                                          # the kernel holds top_p as a float


def kept(row, t, k, p):
    """(mask, probabilities) of the kept tokens: sample_ref.kept_from_scaled's rule (ties are kept whole) on the scaled row."""
    return kept_from_scaled(scaled(row, t, k), k, _p32(p) if p < 1.0 else 1.0)


def kept_band(row, t, k, p, delta):
    """The kept sets at top_p - delta and top_p + delta (each as kept() returns it); one set twice where top-p is off."""
    if p >= 1.0 or k == 1:
        s = kept(row, t, k, p)
        return s, s
    y, p = scaled(row, t, k), _p32(p)
    return kept_from_scaled(y, k, max(p - delta, 1e-300)), kept_from_scaled(y, k, min(p + delta, 1.0))


def draw_delta(row, t, k):
    """bars.draw_cdf_tol on the distribution top-p cuts (temperature and top-k applied): the delta of kept_band."""
    keep, prob = kept(row, t, k, 1.0)
    return cdf_tol(scaled(row, t, k), keep, prob)


def cdf_tol(y, keep, prob):
    import bars
    d = y[keep] - y[keep].max()
    return bars.draw_cdf_tol(prob[keep], d, int(keep.sum()), float(np.exp(d).sum()))


def u24(seed, row, step):
    """sample.hip's uniform: the top 24 bits of hash(hash(seed + row + golden) ^ step), as a multiple of 2^-24."""
    return (h32(h32((int(seed) + int(row) + 0x9E3779B9) & 0xFFFFFFFF) ^ (int(step) & 0xFFFFFFFF)) >> 8) * 2.0 ** -24


def cdf(probs):
    """(kept indices ascending, lower end, upper end) of every kept token's CDF interval, normalised to [0, 1]."""
    idx = np.nonzero(probs > 0)[0]
    c = np.cumsum(probs[idx])
    return idx, (c - probs[idx]) / c[-1], c / c[-1]


def draw_interval(probs, seed, row, step):
    """u and the CDF interval of every kept token in vocabulary-index order: (u, indices, lower ends, upper ends)."""
    return (u24(seed, row, step),) + cdf(probs)


def draw64(u, idx, lo, hi):
    """The float64 draw: the kept token whose interval holds u -> (token, position among the kept)."""
    j = min(int(np.searchsorted(hi, u, side="right")), len(idx) - 1)
    return int(idx[j]), j


def check_draws(row, t, k, p, seed, row_seed, steps, toks):
    """The rule every sample_rows draw is held to, for ONE row and its draws toks[i] at steps[i] -> dict(errors, undecided, undecided_same_sets,
    ratio, tol).  With lo / hi = the kept sets of kept_band (lo within hi: a kernel whose top-p prefix is within delta of the float64 one keeps a
    set between them) and tol = draw_cdf_tol:
      every draw: the token is in lo or hi and u lies in its float64 CDF interval under that set, widened by tol (ratio = the worst distance
        outside the interval / tol);
      decided draws: the token equals the float64 draw.  With A the mass of lo, E that of hi \\ lo, a and b the prefix of lo before and through
        token i, every set between lo and hi puts i's interval inside [a / (A + E), (b + E) / (A + E)] and leaves (a + E) / (A + E) .. b / (A + E)
        to i alone: a draw is decided when u is more than tol inside that core.  Where the two sets are equal (E = 0) the core is the interval
        itself, the plain rule; undecided_same_sets counts by that plain rule alone (a row whose sets differ is then undecided as a whole)."""
    y = scaled(row, t, k)
    (ka, pa), (kb, pb) = kept_band(row, t, k, p, draw_delta(row, t, k))
    tol = max(cdf_tol(y, ka, pa), cdf_tol(y, kb, pb))
    same = bool(np.array_equal(ka, kb))
    sets = [(ka, cdf(pa))] + ([] if same else [(kb, cdf(pb))])
    w = np.where(kb, np.exp(np.where(kb, y, 0.0) - y[ka].max()), 0.0)
    idx = np.nonzero(ka)[0]
    A, E = w[ka].sum(), w[kb & ~ka].sum()
    b = np.cumsum(w[idx])
    core_lo, core_hi = (b - w[idx] + E) / (A + E), b / (A + E)
    out = dict(errors=[], undecided=0, undecided_same_sets=0, ratio=0.0, tol=tol, same=same)
    for st, tok in zip(steps, toks):
        u, tok = u24(seed, row_seed, st), int(tok)
        miss = float("inf")
        for keep, (ix, lo, hi) in sets:
            if 0 <= tok < len(keep) and keep[tok]:
                j = int(np.searchsorted(ix, tok))
                miss = min(miss, max(lo[j] - u, u - hi[j], 0.0))
        if miss == float("inf"):
            out["errors"].append(f"step {st}: token {tok} is in neither kept set")
        elif miss > tol:
            out["errors"].append(f"step {st}: u = {u:.8f} is {miss:.3e} outside token {tok}'s interval (tol {tol:.3e})")
        if miss < float("inf"):
            out["ratio"] = max(out["ratio"], miss / tol)
        j = int(np.searchsorted(core_hi, u, side="right"))
        decided = j < len(idx) and u - core_lo[j] > tol and core_hi[j] - u > tol
        if decided and tok != int(idx[j]):
            out["errors"].append(f"step {st}: decided draw gives token {int(idx[j])}, got {tok}")
        out["undecided"] += not decided
        out["undecided_same_sets"] += not (decided and same)
    return out


def draws64(row, t, k, p, seed, row_seed, steps):
    """The float64 draws of one row (top_p as given, no band)."""
    _, prob = kept(row, t, k, p)
    idx, lo, hi = cdf(prob)
    return [draw64(u24(seed, row_seed, st), idx, lo, hi)[0] for st in steps]


# host emulation: fp32 exponentials, exact integer masses
def masses32(y32, keep):
    """floor(expf32(y - max) * 2^40) of the kept entries as uint64 (0 elsewhere); y32: the float32 scaled row."""
    y32 = np.asarray(y32, np.float32)
    m = y32[keep].max()
    e = np.exp(np.where(keep, y32 - m, np.float32(-np.inf)).astype(np.float32)).astype(np.float32)
    return (e.astype(np.float64) * 2.0 ** 40).astype(np.uint64)


def emul_top_p_keep(y32, keep_k, p):
    """sample.hip's top-p over the top-k survivors with integer masses: the largest threshold whose mass above reaches ceil(top_p * Z)."""
    w = masses32(y32, keep_k)
    Z = int(w.sum())
    target = min(max(int(np.ceil(float(np.float32(p)) * float(Z))), 1), Z)
    order = np.argsort(-np.where(keep_k, y32, -np.inf).astype(np.float64), kind="stable")[: int(keep_k.sum())]
    c = np.cumsum(w[order])
    j = int(np.argmax(c >= target))
    return keep_k & (y32 >= y32[order][j])


def emul_draw(y32, keep, u, shift=0, tile_shift=0, inclusive_bug=False, w=None):
    """sample.hip's draw: W = the exact sum of the masses, target = floor(W u) (clamped below W), the first kept token whose inclusive prefix
    exceeds the target, found as the kernel does: tile sums, an exclusive scan over tiles, then the crossing inside one tile.
    Planted faults: shift (tokens), tile_shift (tiles), inclusive_bug (the tile scan's inclusive prefix used for the exclusive one).  w: the
    masses, where the caller holds them already."""
    w = masses32(y32, keep) if w is None else w
    V = len(w)
    W = int(w.sum())
    target = min(int(float(W) * u), W - 1)
    nt = (V + TILE - 1) // TILE
    ts = np.add.reduceat(w, np.arange(0, V, TILE))
    inc = np.cumsum(ts)
    exc = inc - ts
    t = int(np.argmax((exc <= target) & (target < inc)))
    rel = target - int(inc[t] if inclusive_bug else exc[t])
    t = min(max(t + tile_shift, 0), nt - 1)
    c = np.cumsum(w[t * TILE:(t + 1) * TILE].astype(np.int64))
    hit = np.nonzero(c > rel)[0]
    tok = t * TILE + (int(hit[0]) if len(hit) else 0)
    return min(max(tok + shift, 0), V - 1)


def sample_logprob_ratio(row, t, k, p, toks, lps):
    """max |logprob - float64 log-softmax over the kept set| / select_logprob_bar over one row's draws toks with scores lps; where the band's two
    kept sets differ a draw is held to the nearer of the two.  A NaN or infinite score fails here; a token in neither set gives inf."""
    import bars
    lps = np.asarray(lps, np.float64)
    assert np.isfinite(lps).all(), "a draw's log-probability is NaN or infinite"
    y = scaled(row, t, k)
    best = np.full(len(toks), np.inf)
    for keep, _ in kept_band(row, t, k, p, draw_delta(row, t, k)):
        z = torch.as_tensor(y[keep])
        ref = torch.log_softmax(z, 0)
        cpu = torch.log_softmax(z.float(), 0)
        bar = bars.select_logprob_bar(ref, cpu, int(keep.sum()), sizes=(z, z - z.max(), ref))
        pos = np.searchsorted(np.nonzero(keep)[0], toks)
        err = np.where(keep[toks], np.abs(lps - ref.numpy()[np.minimum(pos, len(ref) - 1)]), np.inf)
        best = np.minimum(best, err / bar)
    return float(best.max())


def sample_logprob64(y64, keep, tok):
    """log-softmax over the kept set at the drawn token, float64."""
    z = y64[keep]
    m = z.max()
    return float(y64[tok] - m - np.log(np.exp(z - m).sum()))


def sample_logprob32(y32, keep, tok):
    """sample.hip's arithmetic: (y - max) - logf(float(W) * 2^-40), W the exact integer mass."""
    W = int(masses32(y32, keep).sum())
    m = np.float32(y32[keep].max())
    return float(np.float32(np.float32(y32[tok]) - m) - np.log(np.float32(np.float32(W) * np.float32(2.0 ** -40))))


# ---------------------------------------------------------------- beam_topk
def log_softmax64(x):
    return torch.log_softmax(torch.as_tensor(x).double(), dim=-1)       # -inf entries stay -inf


def beam_scores64(logits, beam_scores, logprobs=False):
    """beam_scores[r] + log_softmax64(x[r]) (or + x[r] when logprobs), float64 [rows, V]; entries of -inf stay -inf."""
    x = torch.as_tensor(logits).double()
    return torch.as_tensor(beam_scores).double()[:, None] + (x if logprobs else log_softmax64(x))


def beam_scores32(logits, beam_scores, rescale=True, drop_seg=None):
    """beam.hip's arithmetic in float32: per segment of 4096 logits the max and sum exp(x - max), folded as M = max of maxima,
    Z = sum s_seg * exp(m_seg - M), score = bs + ((x - M) - log Z).  Planted faults: rescale=False (a segment's sum not rescaled to the row
    maximum), drop_seg (one segment left out of Z)."""
    x = torch.as_tensor(logits).float()
    rows, V = x.shape
    nseg = (V + SEG - 1) // SEG
    pad = torch.full((rows, nseg * SEG - V), NEG)
    xs = torch.cat([x, pad], 1).view(rows, nseg, SEG)
    m = xs.max(-1).values
    s = torch.where(torch.isinf(xs), torch.zeros_like(xs), torch.exp(xs - m[..., None])).sum(-1)
    M = m.max(-1, keepdim=True).values
    f = torch.exp(m - M) if rescale else torch.ones_like(m)
    part = s * f
    if drop_seg is not None:
        part[:, drop_seg] = 0.0
    Z = part.sum(-1, keepdim=True)
    return torch.as_tensor(beam_scores).float()[:, None] + ((x - M) - torch.log(Z))


def beam_order(score, k):
    """The k best flat indices of one item's scores [nb * V] by a stable host sort on (-score, flat index); score: any float tensor."""
    s = torch.as_tensor(score).double().numpy().ravel()
    if len(s) > 4 * k:                                                   # only the entries at or above the k-th value can be returned
        kth = np.partition(s, len(s) - k)[len(s) - k]
        cand = np.flatnonzero(s >= kth)
    else:
        cand = np.arange(len(s))
    return cand[np.argsort(-s[cand], kind="stable")[:k]]


def beam_valid(got_s, got_flat, score64, k, bar):
    """The validity rule of a beam_topk result for ONE batch item; returns (ok, worst error / bar or the reason).  score64: float64 [nb * V].
      pairs distinct and in range; each returned score within `bar` of the float64 score of its own pair (both -inf: equal); returned scores
      do not increase; equal float32 scores come in ascending flat index; no pair left out scores above the k-th returned pair's float64
      score + 2 bar (one bar for each side of that comparison)."""
    s64 = torch.as_tensor(score64).double().numpy().ravel()
    gs = np.asarray(got_s, np.float32)
    fl = np.asarray(got_flat, np.int64)
    if len(set(fl.tolist())) != k or fl.min() < 0 or fl.max() >= len(s64):
        return False, "pairs not distinct or out of range"
    own = s64[fl]
    inf = np.isinf(own)
    if np.isnan(gs).any():
        return False, "NaN scores"
    if not np.array_equal(np.isinf(gs), inf) or (gs[inf] != own[inf]).any():
        return False, "infinite scores differ"
    err = float(np.abs(gs.astype(np.float64)[~inf] - own[~inf]).max()) if (~inf).any() else 0.0
    if not err <= bar:
        return False, f"score off by {err:.3e} > bar {bar:.3e}"
    if not (gs[1:] <= gs[:-1]).all():
        return False, "scores increase"
    if ((gs[1:] == gs[:-1]) & (fl[1:] < fl[:-1])).any():
        return False, "equal scores not in ascending flat index"
    rest = s64.copy()
    rest[fl] = -np.inf
    if not rest.max() <= own[-1] + 2.0 * bar:
        return False, f"a pair left out scores {rest.max() - own[-1]:.3e} above the k-th returned"
    return True, (err / bar if bar > 0 else 0.0)


# ---------------------------------------------------------------- row_scores
def row_scores64(x, tok, temperature, dtype=F64):
    """(logprob, entropy) per row on the float32 values, the division by the float32 temperature in float32; dtype=float32 gives the host's
    float32 evaluation of the same formula."""
    y = (torch.as_tensor(x).float() / torch.tensor(temperature, dtype=torch.float32)).to(dtype)
    lse = torch.logsumexp(y, dim=1)
    lp = y.gather(1, tok[:, None])[:, 0] - lse
    ent = torch.special.entr(torch.exp(y - lse[:, None])).sum(1)
    return lp, ent


def mst_emul(y32, lanes=1024, skip_raise=False, leave_out=None):
    """token_score.hip's online recurrence in float32 for ONE row: each of `lanes` threads folds its strided share into (m, s, t) =
    (max, sum exp(y - m), sum exp(y - m) (y - m)), raising the state when the maximum moves; the states are merged by a butterfly.
    Returns (m, s, t) as float32 scalars.  Planted faults: skip_raise (merge adds the sums without raising the lower side), leave_out (an index
    whose term is left out of the sums)."""
    f = np.float32
    y = np.asarray(y32, f).copy()
    if leave_out is not None:
        y[leave_out] = -np.inf
    n = -(-len(y) // lanes)
    y = np.concatenate([y, np.full(n * lanes - len(y), -np.inf, f)]).reshape(n, lanes)
    m, s, t = np.full(lanes, -np.inf, f), np.zeros(lanes, f), np.zeros(lanes, f)

    def raise_(m, s, t, mn):
        live = np.isfinite(m) & (mn > m)
        d = np.where(live, m - mn, f(0)).astype(f)
        e = np.exp(d).astype(f)
        t2 = np.where(live, e * (t + s * d), t).astype(f)
        s2 = np.where(live, s * e, s).astype(f)
        return np.maximum(m, mn), s2, t2

    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            m, s, t = raise_(m, s, t, y[i])
            ok = np.isfinite(y[i])
            d = np.where(ok, y[i] - m, f(0)).astype(f)
            e = np.where(ok, np.exp(d), f(0)).astype(f)
            s = (s + e).astype(f)
            t = (t + e * d).astype(f)
        w = lanes
        while w > 1:
            w //= 2
            a, b = (m[:w], s[:w], t[:w]), (m[w:2 * w], s[w:2 * w], t[w:2 * w])
            M = np.maximum(a[0], b[0])
            if not skip_raise:
                a, b = raise_(*a, M), raise_(*b, M)
            m, s, t = M, (a[1] + b[1]).astype(f), (a[2] + b[2]).astype(f)
    return m[0], s[0], t[0]


def mst_scores(m, s, t, y_tok):
    """(logprob, entropy) from a merged state as the kernel forms them, float32."""
    f = np.float32
    ls = np.log(f(s)).astype(f)
    return float(f(f(y_tok) - f(m)) - ls), float(max(f(ls - f(t) / f(s)), f(0)))


def log_softmax32(x):
    """The log-softmax stage of logits_process.hip: three float32 passes (max, sum exp(x - max), (x - max) - log sum)."""
    x = torch.as_tensor(x).float()
    m = x.max(-1, keepdim=True).values
    z = torch.exp(x - m).sum(-1, keepdim=True)
    return (x - m) - torch.log(z)
