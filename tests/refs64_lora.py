"""Plain float64 restatements of the LoRA adapter kernels (csrc/lora_batch.hip: avllm_lora_rank3 and avllm_gemm_tn_multi, each in its shared and
its non-shared form; csrc/lora_dx.hip: avllm_lora_dx_masked) as include/avllm.h and the file headers state them, their input families, a host
emulation of the arithmetic the kernels document with the mutants tests/test_lora_refs_cpu.py builds from it, and the case tables of
tests/test_lora_pin_gpu.py.  The dropout mask, the matrix restatements' building blocks, the families and the comparison are those of
tests/refs64_gemm.py (keep_grid, dropped_operand, drop_scale, family, family_tn, cancel_R, verify, exact_holds); nothing here touches the GPU.

A case (case_rank3 / case_tn / case_dx) is a dict that holds the host operands, the float64 references, the bars and where every output sits
inside its NaN buffer; images() makes the buffers (host float64 for the emulation, device bf16 / fp32 for the kernels), emul() fills host
buffers, check() compares either kind."""
from collections import namedtuple

import torch

import refs64_gemm as G

F64, F32, BF16 = G.F64, G.F32, G.BF16
R0, C0 = 1, 8                                   # where an output starts inside its NaN buffer
SEEDS = (0x5EED1234, 0x0BADC0DE, 0x13579BDF)    # per-adapter seed offsets
WRAP_BASE = 0xFFFFFF00                          # a base seed (the word behind seed_dev) whose sum with every offset above passes 2^32


def eff_seed(base, off):
    """av_seed of common.h: (*seed_dev or 0) + offset in uint32 arithmetic."""
    return (int(base) + int(off)) & 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ the references
def rank3(As, Bs, R, alpha=1.0, seeds=None, p=0.0, shared=False, base=0):
    """C_j [M, 64] = alpha dropout_j(A) B_j[:R]^T, columns >= R zero.  shared: every adapter reads As[0] through its own mask (index row K + col,
    survivors scaled in fp32 and re-rounded to bf16: G.dropped_operand); else adapter j reads As[j], no mask.  Bs[j]: the padded image [>= 16, K_j].
    -> one G.Ref per adapter (what Bar.gemm_bar reads)."""
    refs = []
    for j, B in enumerate(Bs):
        A = As[0] if shared else As[j]
        A_ = G.dropped_operand(A, eff_seed(base, seeds[j]), p) if shared and p > 0 else G._c(A, F64)
        B_ = G._c(B, F64)[:R]
        M = A_.shape[0]
        acc, sa = torch.zeros(M, 64, dtype=F64), torch.zeros(M, 64, dtype=F64)
        acc[:, :R] = A_ @ B_.t()
        sa[:, :R] = A_.abs() @ B_.abs().t()
        z = alpha * acc
        refs.append(G.Ref(z, sa, z, acc, torch.arange(M), None))
    return refs


def tn_multi(Big, Smalls, R, outs0, alpha=1.0, seeds=None, p=0.0, shared=False, cols=None, base=0):
    """shared: out_j [R, NB] = out0_j + alpha Small_j[:, :R]^T dropout_j(Big), mask index row NB + col; else out_j [ncol_j, R] = out0_j + alpha
    Big[:, col0_j : col0_j + ncol_j]^T Small_j[:, :R] with cols = [(col0, ncol), ...].  -> one G.RefTN per adapter."""
    Big_ = G._c(Big, F64)
    refs = []
    for j, S in enumerate(Smalls):
        S_ = G._c(S, F64)[:, :R]
        if shared:
            X = G.dropped_operand(Big, eff_seed(base, seeds[j]), p) if p > 0 else Big_
            acc, sa = S_.t() @ X, S_.abs().t() @ X.abs()
        else:
            X = Big_[:, cols[j][0]:cols[j][0] + cols[j][1]]
            acc, sa = X.t() @ S_, X.abs().t() @ S_.abs()
        refs.append(G.RefTN(alpha * acc + G._c(outs0[j], F64), sa, acc))
    return refs


RefDx = namedtuple("RefDx", "out prods sum_abs keeps scale R")


def dx_masked(Ts, ATs, seeds, r, p, R=None, base=0):
    """out [M, N] = R + sum_j keep(seed_j, m N + n, p) scale (T_j[:, :r] AT_j[:, :r]^T), with the per-adapter products, their sum_abs = |T| |AT|^T
    and the masks the bar needs."""
    M, N = Ts[0].shape[0], ATs[0].shape[0]
    sc = G.drop_scale(p)
    R_ = torch.zeros(M, N, dtype=F64) if R is None else G._c(R, F64)
    out, prods, sas, keeps = R_.clone(), [], [], []
    for j in range(len(Ts)):
        t, a = G._c(Ts[j], F64)[:, :r], G._c(ATs[j], F64)[:, :r]
        prods.append(t @ a.t())
        sas.append(t.abs() @ a.abs().t())
        keeps.append(G.keep_grid(eff_seed(base, seeds[j]), M, N, N, p))
        out = out + torch.where(keeps[j], sc * prods[j], torch.zeros_like(out))
    return RefDx(out, prods, sas, keeps, sc, R_)


def exact_holds(ref, out_bf16):
    """The zero-bar families' condition on the reference alone: the float64 result is representable in the output format."""
    return G.exact_holds(ref) if out_bf16 else bool(torch.equal(ref.out, ref.out.to(F32).to(F64)))


# ------------------------------------------------------------------------------------------------ input families (every value bf16-exact, fp32 tensors)
def _ab(fam, M, K, j):
    """(A [M, K], B [16, K]) of adapter j from G.family; the locate code (the same for every seed) is shifted by j rows so that adapters differ."""
    d = G.family(fam, M, 16, K, seed=j)
    B = G.locate_code(16 + j, K)[j:].contiguous() if fam == "locate" else d["B"]
    return d["A"], B


def pad_rows(B, R):
    B = B.clone()
    B[R:] = 0
    return B


def pad_cols(S, R):
    S = S.clone()
    S[:, R:] = 0
    return S


def family_dx(fam, M, N, r, nj):
    """Ts nj x [M, r], ATs nj x [N, r], R [M, N].  exact: T has min(r, 4) entries of +-1 per row, AT in {+-1, +-2}: |product| <= 8, so that
    2 * 3 * 8 + |R| <= 56 is a bf16 integer.  locate: T one-hot at column (m + j) % r, AT an integer code of (n, column, j) with |code| <= 41:
    2 * 3 * 41 + 8 = 254 <= 256."""
    Ts, ATs = [], []
    g = G._gen("dx", fam, M, N, r, nj)
    for j in range(nj):
        if fam in ("randn", "offset", "heavy"):
            d = G.family(fam, M, N, r, seed=j)
            t, a = d["A"], d["B"]
        elif fam == "exact":
            nnz = min(r, 4)
            t = torch.zeros(M, r)
            cols = torch.rand(M, r, generator=g).argsort(1)[:, :nnz]
            t.scatter_(1, cols, (torch.randint(0, 2, (M, nnz), generator=g) * 2 - 1).to(F32))
            a = (torch.randint(1, 3, (N, r), generator=g) * (torch.randint(0, 2, (N, r), generator=g) * 2 - 1)).to(F32)
        else:
            t = torch.zeros(M, r)
            t[torch.arange(M), (torch.arange(M) + j) % r] = 1.0
            n, c = torch.arange(N)[:, None], torch.arange(r)[None, :]
            a = (((3 * n + 7 * c + 13 * j) % 83) - 41).to(F32)
        Ts.append(G._bf(t))
        ATs.append(G._bf(a))
    R = G.family(fam, M, N, r)["R"] if fam in ("randn", "offset", "heavy") else torch.randint(-8, 9, (M, N), generator=g).to(F32)
    return Ts, ATs, G._bf(R)


# ------------------------------------------------------------------------------------------------ case tables of the GPU file
# Every table row is run at every edge M of its form and in every family; "p" stands for G.drop_p(family): 0.5 in the zero-bar families (the scale 2
# is exact), 0.05 elsewhere.  base != 0: the base seed sits in device memory (seed_dev) and base + offset wraps 2^32.
RK_M = (1, 15, 16, 17, 50)                       # one row, one short of / exactly / one past the 16-row workgroup, several workgroups with a tail
RK_SHARED = (                                    # K, nj, R, p, alpha, layout, base.  K / 8 per wave = 32 (tail only), 64 (tail x 2), 128 (unrolled
    (256, 1, 1, 0.0, 2.0, "sep", 0),             # only), 160 (unrolled + tail).  layout "one": 64-column slices of one buffer; "sep": one each
    (512, 2, 8, "p", 0.5, "one", 0),
    (1024, 3, 16, "p", 2.0, "one", 0),
    (1280, 3, 16, "p", 0.5, "sep", WRAP_BASE),
    (1280, 2, 8, 0.0, 2.0, "one", 0),
)
RK_SPLIT_K = (1280, 256, 512)                    # adapter j's K: column slices of one [M, 2048] buffer, so lda = 2048 != K
RK_SPLIT = ((1, 16, 2.0, "one"), (2, 8, 0.5, "sep"), (3, 1, 2.0, "one"), (3, 16, 0.5, "sep"))          # nj, R, alpha, layout

TN_M = (1, 63, 64, 65, 300, 700, 8300)           # a slab with a tail, the exact slab, two slabs, chunks with a ragged last one, the 32-chunk cap
TN_SHARED = (                                    # NB, nj, R, p, alpha, base
    (128, 1, 1, 0.0, 1.0, 0),
    (384, 2, 8, "p", 0.5, 0),
    (128, 3, 16, "p", 1.0, 0),
    (384, 3, 16, 0.0, 0.5, 0),
    (128, 2, 8, "p", 1.0, WRAP_BASE),
)
TN_SPLIT = (((128,), 1, 1.0), ((128, 128), 8, 0.5), ((256, 128, 128), 16, 1.0), ((128, 256, 128), 8, 0.5))          # ranges, R, alpha

DX_M = (1, 31, 32, 33, 127, 128, 129, 200)       # the 32-row wave and the 128-row workgroup, one short of / exactly / one past, two workgroups
DX = (                                           # N, nj, r, p, ld, R, base.  ld: row stride of T and AT (32, 64) or "slice" = 64-column slices of
    (128, 1, 4, 0.0, 32, "none", 0),             # a 192-wide buffer.  R: "none", "sep" (its own tensor) or "alias" (R is out)
    (384, 2, 16, "p", 64, "sep", 0),
    (128, 3, 32, "p", "slice", "alias", 0),
    (384, 3, 16, "p", 32, "alias", WRAP_BASE),
    (128, 2, 32, 0.0, 64, "sep", 0),
)


def shared_big_m(M, NB):
    """The issue's one exclusion: M = 8300 runs the shared form at NB = 128 only."""
    return not (M == 8300 and NB != 128)


def _p(p, fam):
    return G.drop_p(fam) if p == "p" else p


def tn_chunks(M, want):
    """tn_chunks of lora_batch.hip: at most 32 chunks of whole 64-row slabs.  -> (chunks, rows per chunk)"""
    zs = min(32, -(-M // want))
    mchunk = -(-(-(-M // zs)) // 64) * 64
    return -(-M // mchunk), mchunk


def case_rank3(fam, M, row, shared):
    import bars as Bar
    if shared:
        K, nj, R, p, alpha, layout, base = row
        p = _p(p, fam)
        As = [_ab(fam, M, K, 0)[0]]
        Bs = [pad_rows(_ab(fam, M, K, j)[1], R) for j in range(nj)]
        Ks = [K] * nj
    else:
        (nj, R, alpha, layout), p, base = row, 0.0, 0
        Ks = list(RK_SPLIT_K[:nj])
        ab = [_ab(fam, M, Ks[j], j) for j in range(nj)]
        As, Bs = [x[0] for x in ab], [pad_rows(x[1], R) for x in ab]
    seeds = list(SEEDS[:nj])
    refs = rank3(As, Bs, R, alpha, seeds, p, shared, base)
    bars = [0.0 if fam in G.ZERO_BAR else Bar.lora_rank3_bar(refs[j], Ks[j], alpha) for j in range(nj)]
    if layout == "one":
        shapes, slots = [(M + R0 + 3, 64 * nj + 16)], [(0, R0, C0 + 64 * j, M, 64) for j in range(nj)]
    else:
        shapes, slots = [(M + R0 + 3, 80)] * nj, [(j, R0, C0, M, 64) for j in range(nj)]
    return dict(kind="rank3", fam=fam, M=M, As=As, Bs=Bs, Ks=Ks, R=R, nj=nj, p=p, alpha=alpha, seeds=seeds, base=base, shared=shared, refs=refs,
                bars=bars, shapes=shapes, slots=slots, out_bf16=True, init=None, sentinel=None)


def case_tn(fam, M, row, shared, padded=True, sentinel=None):
    """padded=False, sentinel=x: the guard case.  Small keeps values past column R (the kernel reads 16 columns and must store R) and the buffer
    around the output holds the finite x instead of NaN: a float atomic onto NaN stays NaN, onto x it shows."""
    import bars as Bar
    if shared:
        NB, nj, R, p, alpha, base = row
        p, cols = _p(p, fam), None
    else:
        (ranges, R, alpha), p, base = row, 0.0, 0
        nj, NB = len(ranges), sum(ranges)
        cols = [(sum(ranges[:j]), ranges[j]) for j in range(nj)]
    big, q, o = G.family_tn(fam, M, NB, 16 * nj)
    sm = [q[:, 16 * j:16 * j + 16] for j in range(nj)]
    Smalls = [pad_cols(s, R) if padded else s.clone() for s in sm]
    if shared:
        outs0 = [o[:, 16 * j:16 * j + R].t().contiguous() for j in range(nj)]
        shapes, slots = [(R0 + 16 + 3, NB + 16)] * nj, [(j, R0, C0, R, NB) for j in range(nj)]
    else:
        outs0 = [o[c0:c0 + nc, 16 * j:16 * j + R].contiguous() for j, (c0, nc) in enumerate(cols)]
        shapes, slots = [(nc + R0 + 3, 32) for _, nc in cols], [(j, R0, C0, nc, R) for j, (_, nc) in enumerate(cols)]
    seeds = list(SEEDS[:nj])
    refs = tn_multi(big, Smalls, R, outs0, alpha, seeds, p, shared, cols, base)
    bars = [0.0 if fam in G.ZERO_BAR else Bar.lora_tn_multi_bar(refs[j], M, alpha, outs0[j].double()) for j in range(nj)]
    return dict(kind="tn", fam=fam, M=M, NB=NB, Big=big, ldb=NB + 24, Smalls=Smalls, R=R, nj=nj, p=p, alpha=alpha, seeds=seeds, base=base, shared=shared,
                cols=cols, refs=refs, bars=bars, shapes=shapes, slots=slots, out_bf16=False, init=outs0, sentinel=sentinel)


def case_dx(fam, M, row):
    import bars as Bar
    N, nj, r, p, ld, rmode, base = row
    p = _p(p, fam)
    Ts, ATs, R = family_dx(fam, M, N, r, nj)
    seeds = list(SEEDS[:nj])
    if rmode == "none":
        R = None
    elif fam == "offset":                         # the single-rounding check: R cancels the masked sum to size 1
        R = G.cancel_R(dx_masked(Ts, ATs, seeds, r, p, None, base).out, M)
    ref = dx_masked(Ts, ATs, seeds, r, p, R, base)
    bar = 0.0 if fam in G.ZERO_BAR else Bar.lora_dx_bar(ref)
    return dict(kind="dx", fam=fam, M=M, N=N, Ts=Ts, ATs=ATs, Rt=R, r=r, nj=nj, p=p, ld=ld, rmode=rmode, seeds=seeds, base=base, refs=[ref], bars=[bar],
                shapes=[(M + R0 + 3, N + 16)], slots=[(0, R0, C0, M, N)], out_bf16=True, init=[R] if rmode == "alias" else None, sentinel=None)


def zero_bar_ok(c):
    return all(exact_holds(ref, c["out_bf16"]) for ref in c["refs"])


# ------------------------------------------------------------------------------------------------ buffers and the comparison
def images(c, device="cpu", dtype=None):
    """-> (bufs, outs): one buffer per group, NaN (or the case's sentinel) everywhere, prior values copied into the outputs that have some; outs[j]
    = adapter j's output view.  Host images are float64 (they hold the emulation's bf16 / fp32 values exactly)."""
    if dtype is None:
        dtype = F64 if device == "cpu" else (BF16 if c["out_bf16"] else F32)
    fill = float("nan") if c["sentinel"] is None else c["sentinel"]
    bufs = [torch.full(shape, fill, device=device, dtype=dtype) for shape in c["shapes"]]
    outs = []
    for j, (g, r0, c0, rows, cols) in enumerate(c["slots"]):
        v = bufs[g][r0:r0 + rows, c0:c0 + cols]
        if c["init"] is not None:
            v.copy_(c["init"][j].to(dtype))
        outs.append(v)
    return bufs, outs


def check(c, bufs):
    """G.verify over every buffer of the case -> (canaries overwritten, elements beyond the bar, worst error / bar)."""
    canary = over = 0
    worst = 0.0
    for g in range(len(bufs)):
        js = [j for j, s in enumerate(c["slots"]) if s[0] == g]
        _, r0, c0, rows, _ = c["slots"][js[0]]
        ref = torch.cat([c["refs"][j].out for j in js], 1).to(bufs[g].device)
        bar = c["bars"][js[0]]
        if torch.is_tensor(bar):
            bar = torch.cat([c["bars"][j] for j in js], 1).to(bufs[g].device)
        b = bufs[g].to(F64)
        if c["sentinel"] is not None:             # a finite border: what still holds the sentinel outside the output counts as untouched
            outside = torch.ones(b.shape, dtype=torch.bool, device=b.device)
            outside[r0:r0 + rows, c0:c0 + ref.shape[1]] = False
            b = torch.where(outside & (b == c["sentinel"]), torch.full_like(b, float("nan")), b)
        ca, ov, ra = G.verify(b, r0, c0, torch.arange(rows, device=b.device), ref.shape[1], ref, bar)
        canary, over, worst = canary + ca, over + ov, max(worst, ra)
    return canary, over, worst


# ------------------------------------------------------------------------------------------------ host emulation of the documented arithmetic
MUTANTS = ("seed0_all", "mask_stride", "no_scale", "pad_unwritten", "slab_tail", "range_neighbour", "rows_ge_R", "round_per_adapter", "mask_after_R",
           "seed_dev_ignored")
_f = G._f


def _masked32(X, seed, p, stride, mut):
    """The fused mask of an operand in fp32 -> fp32 tensor of bf16 values."""
    if mut == "no_scale":
        X32 = G._c(X, F32)
        return torch.where(G.keep_grid(seed, X32.shape[0], X32.shape[1], stride, p), X32, torch.zeros_like(X32))
    return G.dropped_operand(X, seed, p, stride).to(F32)


def _seed(c, j, mut):
    return eff_seed(0 if mut == "seed_dev_ignored" else c["base"], c["seeds"][0 if mut == "seed0_all" else j])


def emul_rank3(c, bufs, mut=None):
    """fp32 partials per wave over K / 8, added in wave order, times alpha, one bf16 rounding; all 16 rows of B are read and summed, columns 16..63
    are written as zeros."""
    for j in range(c["nj"]):
        A = c["As"][0 if c["shared"] else j]
        K = c["Ks"][j]
        A32 = _masked32(A, _seed(c, j, mut), c["p"], K, mut) if c["shared"] and c["p"] > 0 else G._c(A, F32)
        B32 = G._c(c["Bs"][j], F32)[:16]
        kw = K // 8
        s = torch.zeros(A32.shape[0], 16, dtype=F32)
        for w in range(8):
            s = s + A32[:, w * kw:(w + 1) * kw] @ B32[:, w * kw:(w + 1) * kw].t()
        v = torch.zeros(A32.shape[0], 64, dtype=F32)
        v[:, :16] = s * _f(c["alpha"])
        g, r0, c0, rows, cols = c["slots"][j]
        ncol = c["R"] if mut == "pad_unwritten" else 64
        bufs[g][r0:r0 + rows, c0:c0 + ncol] = v.to(BF16).to(F64)[:, :ncol]


def emul_tn(c, bufs, mut=None):
    """64-row slabs (rows >= M of the last one are zeros), one fp32 partial per chunk and adapter, times alpha, added in chunk order onto the prior
    output (the float atomics' arrival order is not fixed; the bar covers any)."""
    M, R = c["M"], c["R"]
    zs, mchunk = tn_chunks(M, 256 if c["shared"] else 512)
    Big32 = G._c(c["Big"], F32)
    for j in range(c["nj"]):
        S32 = G._c(c["Smalls"][j], F32)[:, :16]
        if c["shared"]:
            X = Big32
            if c["p"] > 0:
                X = _masked32(c["Big"], _seed(c, j, mut), c["p"], c["ldb"] if mut == "mask_stride" else c["NB"], mut)
        else:
            X = Big32[:, c["cols"][j][0]:c["cols"][j][0] + c["cols"][j][1]]
        g, r0, c0, rows, cols = c["slots"][j]
        nr = 16 if mut == "rows_ge_R" else R
        tot = bufs[g][r0:r0 + (nr if c["shared"] else rows), c0:c0 + (cols if c["shared"] else nr)].to(F32)
        for z in range(zs):
            m_begin, m_end = z * mchunk, min(M, (z + 1) * mchunk)
            acc = torch.zeros(nr, X.shape[1], dtype=F32)
            for mb in range(m_begin, m_end, 64):
                idx = torch.arange(mb, min(mb + 64, m_end))
                if mut == "slab_tail" and mb + 64 > m_end:                       # the staging registers still hold the previous slab's rows
                    idx = torch.arange(mb, mb + 64)
                    idx = torch.where(idx < m_end, idx, (idx - 64).clamp_min(0))
                acc = acc + S32[idx, :nr].t() @ X[idx]
            part = _f(c["alpha"]) * acc
            if mut == "range_neighbour" and not c["shared"] and j > 0:          # the range's first 128-column tile went to adapter j - 1's output
                part[:, :128] = 0
            tot = tot + (part if c["shared"] else part.t())
        bufs[g][r0:r0 + tot.shape[0], c0:c0 + tot.shape[1]] = tot.to(F64)


def emul_dx(c, bufs, mut=None):
    """Per adapter one product from a zero accumulator, mask and scale in fp32, summed in adapter order, + R, one bf16 rounding."""
    M, N, nj = c["M"], c["N"], c["nj"]
    g, r0, c0, rows, cols = c["slots"][0]
    R32 = None
    if c["rmode"] == "alias":
        R32 = bufs[g][r0:r0 + M, c0:c0 + N].to(F32)
    elif c["rmode"] == "sep":
        R32 = G._c(c["Rt"], F32)
    sc = _f(1.0 if mut == "no_scale" else G.drop_scale(c["p"]))
    acc = torch.zeros(M, N, dtype=F32)
    for j in range(nj):
        pj = G._c(c["Ts"][j], F32) @ G._c(c["ATs"][j], F32).t()
        k = G.keep_grid(_seed(c, j, mut), M, N, bufs[g].shape[1] if mut == "mask_stride" else N, c["p"])
        v = pj * sc
        if mut == "mask_after_R" and j == nj - 1 and R32 is not None:          # R rides under the last adapter's mask
            v, R32 = v + R32, None
        v = torch.where(k, v, torch.zeros_like(v))
        if mut == "round_per_adapter":
            v = v.to(BF16).to(F32)
        acc = acc + v
    if R32 is not None:
        acc = acc + R32
    bufs[g][r0:r0 + M, c0:c0 + N] = acc.to(BF16).to(F64)


def emul(c, bufs, mut=None):
    {"rank3": emul_rank3, "tn": emul_tn, "dx": emul_dx}[c["kind"]](c, bufs, mut)
    return bufs


# ------------------------------------------------------------------------------------------------ what the GPU file runs, case by case
TN_GUARD_M = (65, 300)
TN_GUARD = ((True, (128, 3, 8, "p", 0.5, 0)), (False, ((128, 128), 8, 0.5)))
SENTINEL = 12345.0


def cases_rank3(M):
    for shared, table in ((True, RK_SHARED), (False, RK_SPLIT)):
        for row in table:
            for fam in G.FAMILIES:
                yield case_rank3(fam, M, row, shared), f"rank3 {'shared' if shared else 'split'} M={M} {row} {fam}"


def cases_tn(M):
    for shared, table in ((True, TN_SHARED), (False, TN_SPLIT)):
        for row in table:
            if shared and not shared_big_m(M, row[0]):
                continue
            for fam in G.FAMILIES:
                yield case_tn(fam, M, row, shared), f"tn_multi {'shared' if shared else 'split'} M={M} {row} {fam}"


def cases_tn_guard(M):
    for shared, row in TN_GUARD:
        for fam in G.FAMILIES:
            yield case_tn(fam, M, row, shared, padded=False, sentinel=SENTINEL), f"tn_multi guard {'shared' if shared else 'split'} M={M} {row} {fam}"


def cases_dx(M):
    for row in DX:
        for fam in G.FAMILIES:
            yield case_dx(fam, M, row), f"lora_dx M={M} {row} {fam}"
