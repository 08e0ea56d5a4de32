"""The LoRA adapter kernels (csrc/lora_batch.hip: avllm_lora_rank3, avllm_gemm_tn_multi, each shared and non-shared; csrc/lora_dx.hip:
avllm_lora_dx_masked) against the float64 restatements of tests/refs64_lora.py, at every launch form (1, 2, 3 adapters; mask or none; seed_dev
null or a device word), every rank padding and the kernels' own edges in M and K.  Bars: tests/bars.py ("LoRA adapter kernels against float64");
none is taken from a kernel's output, the exact and locate families carry the bar 0, and tests/test_lora_refs_cpu.py shows on the host that the
documented arithmetic stays under each while ten mutants do not.

Every output is a view (row 1, column 8 on) of a larger NaN buffer with a row stride wider than the output and spare rows: afterwards everything
outside the output must still be NaN.  The dropout masks are the numpy restatement of common.h (refs64_gemm.keep), never another kernel.  Every
B, T and Small operand is the padded image the contract asks for (zeros past the rank); whatever lies beyond the columns a kernel may read is NaN.
A float atomic onto a NaN border leaves NaN, so gemm_tn_multi also runs guard cases: Small keeps values past column R and the border holds a
finite sentinel that any stray accumulation moves.  Each test prints "RATIO entry form family worst"."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

import refs64_gemm as G  # noqa: E402
import refs64_lora as RL  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
RATIOS = collections.defaultdict(float)


def dev_(t):
    return t.to(BF16).cuda()


def in_nan(t, width, col0=0, read=None):
    """t [rows, c] -> columns col0 .. col0 + read of a NaN [rows, width] bf16 buffer on the GPU; t in the first c of them, zeros up to `read`
    (the columns the kernel may read), NaN everywhere else."""
    read = t.shape[1] if read is None else read
    wide = torch.full((t.shape[0], width), NAN, device="cuda", dtype=BF16)
    view = wide[:, col0:col0 + read]
    view.zero_()
    view[:, :t.shape[1]].copy_(t.to(BF16))
    return view


def slices_of(ts, width, step, read):
    """ts[j] -> columns step j .. step j + read of ONE NaN [rows, width] buffer."""
    wide = torch.full((ts[0].shape[0], width), NAN, device="cuda", dtype=BF16)
    views = []
    for j, t in enumerate(ts):
        v = wide[:, step * j:step * j + read]
        v.zero_()
        v[:, :t.shape[1]].copy_(t.to(BF16))
        views.append(v)
    return views


def seed_word(base):
    """(tensor that owns the device word, the pointer the entries take) or (None, None): the base seed in device memory, as under graph replay."""
    if not base:
        return None, None
    w = torch.tensor([base - (1 << 32) if base >= (1 << 31) else base], dtype=torch.int32, device="cuda")
    return w, L.ptr(w)


def launch(c):
    bufs, outs = RL.images(c, "cuda")
    word, sd = seed_word(c["base"])
    if c["kind"] == "rank3":
        if c["shared"]:
            As = [dev_(c["As"][0])]                                                   # the fused mask wants the contiguous [M, K] activation
        else:
            wide = torch.full((c["M"], 2048), NAN, device="cuda", dtype=BF16)
            As, off = [], 0
            for A in c["As"]:
                As.append(wide[:, off:off + A.shape[1]])
                As[-1].copy_(A.to(BF16))
                off += A.shape[1]
        ops.lora_rank3(As, [dev_(B) for B in c["Bs"]], outs, c["R"], alpha=c["alpha"], seeds=c["seeds"], p=c["p"], shared=c["shared"], seed_dev=sd)
    elif c["kind"] == "tn":
        big = in_nan(c["Big"], c["ldb"], 8)
        smalls = slices_of(c["Smalls"], 192, 64, 16)
        ops.gemm_tn_multi(big, smalls, outs, c["R"], alpha=c["alpha"], seeds=c["seeds"], p=c["p"], shared=c["shared"], cols=c["cols"], seed_dev=sd)
    else:
        if c["ld"] == "slice":
            Ts, ATs = slices_of(c["Ts"], 192, 64, 32), slices_of(c["ATs"], 192, 64, 32)
        else:
            Ts, ATs = [in_nan(t, c["ld"], 0, 32) for t in c["Ts"]], [in_nan(t, c["ld"], 0, 32) for t in c["ATs"]]
        R = None if c["rmode"] == "none" else outs[0] if c["rmode"] == "alias" else in_nan(c["Rt"], c["N"] + 24, 8)
        ops.lora_dx_masked(Ts, ATs, c["seeds"], c["r"], c["p"], R=R, out=outs[0], seed_dev=sd)
    torch.cuda.synchronize()
    del word
    return RL.check(c, bufs)


def run_all(cases, entry):
    """Collects every failure of the parametrised case before asserting."""
    bad, n = [], 0
    for c, what in cases:
        if c["fam"] in G.ZERO_BAR:
            assert RL.zero_bar_ok(c), what
        canary, over, ratio = launch(c)
        n += 1
        if canary or over:
            bad.append(f"{what}: {over} beyond the bar (worst {ratio:.2f}x), {canary} canaries overwritten")
        else:
            form = ("shared" if c["shared"] else "split") if "shared" in c else "-"
            RATIOS[(entry, form, c["fam"])] = max(RATIOS[(entry, form, c["fam"])], ratio)
    print(f"CALLS {n}")
    for key in sorted(RATIOS):
        if key[0] == entry:
            print("RATIO", *key, f"{RATIOS[key]:.3f}")
    assert not bad, f"{len(bad)}/{n} calls failed:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("M", RL.RK_M)
def test_rank3(dev, M):
    run_all(RL.cases_rank3(M), "rank3")


@pytest.mark.parametrize("M", RL.TN_M)
def test_gemm_tn_multi(dev, M):
    run_all(RL.cases_tn(M), "tn_multi")


@pytest.mark.parametrize("M", RL.TN_GUARD_M)
def test_gemm_tn_multi_guard(dev, M):
    """Small with values past column R, a finite border: rows / columns >= R of an output must not be accumulated into."""
    run_all(RL.cases_tn_guard(M), "tn_multi_guard")


@pytest.mark.parametrize("M", RL.DX_M)
def test_lora_dx_masked(dev, M):
    run_all(RL.cases_dx(M), "lora_dx")


# ------------------------------------------------------------------------------------------------ refusals stay refusals, and launch nothing
def test_refusals(dev):
    z = lambda *s: torch.zeros(*s, device="cuda", dtype=BF16)
    out = [torch.full((16, 64), NAN, device="cuda", dtype=BF16) for _ in range(2)]
    with pytest.raises(ValueError, match="lora_rank3"):
        ops.lora_rank3([z(16, 128)], [z(16, 128)], out[:1], 16, shared=True)                                  # K = 128: not 8 waves x 32
    with pytest.raises(ValueError, match="lora_rank3"):
        ops.lora_rank3([z(16, 256), z(16, 256)], [z(16, 256), z(16, 256)], out, 16, seeds=[1, 2], p=0.05)    # a mask on the non-shared form
    assert all(bool(torch.isnan(o.float()).all()) for o in out)
    o32 = [torch.full((128, 16), NAN, device="cuda", dtype=F32) for _ in range(2)]
    small = [z(64, 16), z(64, 16)]
    with pytest.raises(ValueError, match="gemm_tn_multi"):
        ops.gemm_tn_multi(z(64, 256), small, o32, 16, seeds=[1, 2], p=0.05, cols=[(0, 128), (128, 128)])      # a mask on the non-shared form
    with pytest.raises(ValueError, match="gemm_tn_multi"):
        ops.gemm_tn_multi(z(64, 384), small, o32, 16, cols=[(0, 128), (256, 128)])                            # a gap between the ranges
    with pytest.raises(ValueError, match="gemm_tn_multi"):
        ops.gemm_tn_multi(z(64, 384), small, o32, 16, cols=[(0, 128), (128, 128)])                            # the ranges stop short of NB
    with pytest.raises(ValueError, match="gemm_tn_multi"):
        ops.gemm_tn_multi(z(64, 256), small, o32, 16, cols=[(0, 192), (192, 64)])                             # ranges off the 128-column unit
    wide = [torch.full((16, 192), NAN, device="cuda", dtype=F32) for _ in range(2)]
    with pytest.raises(ValueError, match="gemm_tn_multi"):
        ops.gemm_tn_multi(z(64, 192), small, wide, 16, shared=True)                                          # NB = 192
    assert all(bool(torch.isnan(o).all()) for o in o32 + wide)
    dx = torch.full((32, 192), NAN, device="cuda", dtype=BF16)
    with pytest.raises(ValueError, match="lora_dx_masked"):
        ops.lora_dx_masked([z(32, 32)], [z(192, 32)], [1], 16, 0.05, out=dx)                                  # N = 192
    dx2 = torch.full((32, 128), NAN, device="cuda", dtype=BF16)
    with pytest.raises(ValueError, match="lora_dx_masked"):
        ops.lora_dx_masked([z(32, 64)], [z(128, 64)], [1], 33, 0.05, out=dx2)                                 # r = 33
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx.float()).all()) and bool(torch.isnan(dx2.float()).all())
