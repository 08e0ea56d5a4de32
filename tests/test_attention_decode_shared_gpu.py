"""The shared-prefix single-token attention (csrc/attention_decode_shared.hip: ops.attention_decode_shared and its _kv8 twin) against float64.

Inputs are built per item (prefix [B, S]) and per row (suffix [R, n + 1]); the reference is refs64_attention.attn_fwd64 on each row's
concatenation (prefix of item r // group, then the row's suffix), which is what an R-row copy cache holds.  Bars: those of
test_attention_pin_gpu.py::test_decode -- attn_out_bar with no P-rounding term (attn_count_out_bar for the count family), plus
attn_decode_weight_term(S + n + 1, v) outside the count family -- and for the e4m3 form the same on the reference formed from the codes read
(test_kv8_kernels_gpu.py::test_attention_over_the_image).  No number comes from the kernel's output.

Families: count (all scores 0, V small integers that differ per item and per row: a wrong item, a row of another beam, a prefix row skipped or
read twice, or a suffix row past n each change the mean) and offset (V = N(8, 1): the general sum).  Prefix rows past S and suffix rows past n
are NaN (e4m3: code 0x7F, exponent 0xFF)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import bars as Bar  # noqa: E402
import refs64_attention as A  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402
from oracle import mxfp8  # noqa: E402
from test_attention_pin_gpu import check  # noqa: E402

BF = torch.bfloat16
N_SUF = 70                       # suffix cache rows: n = N - 1 takes the suffix launch past one trip of the bf16 hd-128 form and past a pass of all


# The dispatcher has two forms (launch_shared / sh_nsplit in the .hip file).
# Two launches, 4 waves each: a pass covers 256 / (hd / 8) rows of a bf16 cache and 256 / (hd / 16) rows of an e4m3 image, a trip is 4 passes:
#   bf16  hd 128: 64 rows    hd 64: 128 rows          e4m3  hd 128: 128 rows    hd 64: 256 rows
# and the prefix is cut into nsplit = min(16, ceil(S / trip), resident workgroups of the chip / (B ceil(group / 4) H)) slices of ceil(S / nsplit)
# rows.  It is chosen where B ceil(group / 4) H ceil(S / trip) reaches the chip's resident workgroups (512 at the least), which the shapes of
# this file (B ceil(group / 4) H <= 48) do not, so the walk below forces it through the knob SHARED_SPLIT with the count the first two terms give:
# one slice up to a trip, two from one row above it, sixteen from fifteen trips + 1 on.  test_dispatcher_picks_two_launches has the dispatcher
# itself choose it, with the third term binding.
# One launch, 16 waves, prefix and suffix as one sequence of S + n + 1 keys (what the dispatcher picks for every shape here; knob -1 forces it):
# a trip is 4 passes of 1024 / (hd / 8) or 1024 / (hd / 16) rows, four times the lengths above.
def trip_of(form, hd, waves=4):
    return 4 * waves * 64 // (hd // (8 if form == "bf16" else 16))


def s_values(form, hd):
    t = trip_of(form, hd)
    return [1, t - 1, t, t + 1, 16 * t - 1, 16 * t, 16 * t + 1]


def slices_of(form, hd, S):
    t = trip_of(form, hd)
    return min(16, (S + t - 1) // t)


# Every S is run with group 1 and group 2 (kernels of their own) and with one group of the 4-query kernel: 3 and 4 (with and without an idle
# slot), 5 and 8 (a second pass over the slice) in turn.  B = 1 and 3 and n = 0, 1, N - 1 in turn; R <= 16.
FOUR = (4, 3, 5, 8, 4, 3, 5)
NS = (0, 1, N_SUF - 1)


def walk(S_all):
    for i, S in enumerate(S_all):
        for j, group in enumerate((1, 2, FOUR[i % len(FOUR)])):
            yield S, (1 if group == 8 or (i + j) % 2 else 3), group, NS[(i + j) % 3]


def make_inputs(fam, B, group, S, n, H, Hkv, hd, seed):
    """-> q [R, H hd], kp, vp [B, S, dkv], ks, vs [R, n + 1, dkv] bf16 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    R, dkv = B * group, Hkv * hd
    q = torch.randn(R, H * hd, generator=g)
    kp, ks = torch.randn(B, S, dkv, generator=g), torch.randn(R, n + 1, dkv, generator=g)
    if fam == "count":
        kp, ks = torch.zeros_like(kp), torch.zeros_like(ks)
        vp = torch.randint(-4, 5, (B, S, dkv), generator=g).float() + (torch.arange(B).float()[:, None, None] % 3 - 1)
        vs = torch.randint(-4, 5, (R, n + 1, dkv), generator=g).float() + (torch.arange(R).float()[:, None, None] % 5 - 2)
        head = (torch.arange(Hkv).float() % 3 - 1).repeat_interleave(hd)                  # a wrong kv head shows
        vp, vs = vp + head, vs + head
    else:
        vp, vs = torch.randn(B, S, dkv, generator=g) + 8.0, torch.randn(R, n + 1, dkv, generator=g) + 8.0
    return tuple(t.to(BF) for t in (q, kp, vp, ks, vs))


def nan_cache(x, T, form):
    """x [rows, t, dkv] bf16 -> (the cache [rows, T, dkv] in `form` with x in rows [0, t) and NaN after them, the values the kernel reads of x)."""
    rows, t, dkv = x.shape
    if form == "bf16":
        c = torch.full((rows, T, dkv), float("nan"), dtype=BF)
        c[:, :t] = x
        return c, x
    cq, ce = mxfp8.quantize(x.reshape(rows * t, dkv).float())
    codes = torch.full((rows, T, dkv), 0x7F, dtype=torch.uint8)
    exps = torch.full((rows, T, dkv // 32), 0xFF, dtype=torch.uint8)
    codes[:, :t], exps[:, :t] = cq.view(rows, t, dkv), (ce + 127).to(torch.uint8).view(rows, t, dkv // 32)
    return ops.kv8_pack(codes, exps), mxfp8.dequantize(cq, ce).view(rows, t, dkv)


class Case:
    pass


def case(form, fam, B, group, S, n, H, Hkv, hd, same=None):
    """Device inputs, the float64 output of every row over its concatenation and the bar.  same = (r0, r1): row r1 gets q and suffix of row r0."""
    c = Case()
    q, kp, vp, ks, vs = make_inputs(fam, B, group, S, n, H, Hkv, hd, seed=S + 7 * n + 13 * group + B + hd + H)
    if same:
        q[same[1]], ks[same[1]], vs[same[1]] = q[same[0]], ks[same[0]], vs[same[0]]
    R, Tk = B * group, S + n + 1
    (kpc, kpr), (vpc, vpr) = nan_cache(kp, S + 3, form), nan_cache(vp, S + 3, form)
    (ksc, ksr), (vsc, vsr) = nan_cache(ks, N_SUF, form), nan_cache(vs, N_SUF, form)
    item = torch.arange(R) // group
    k_all = torch.cat([kpr[item].float(), ksr.float()], 1).reshape(R * Tk, -1)
    v_all = torch.cat([vpr[item].float(), vsr.float()], 1).reshape(R * Tk, -1)
    args = (R, 1, Tk, H, Hkv, hd, False, hd ** -0.5)
    c.o64 = A.attn_fwd64(q, k_all, v_all, *args)[0]
    if fam == "count":
        c.bar = Bar.attn_count_out_bar(c.o64, True)
    else:
        o32 = A.attn_fwd64(q, k_all, v_all, *args, dtype=torch.float32)[0]
        c.bar = Bar.attn_out_bar(c.o64, None, Bar.fp32_bar(c.o64, o32), True) + Bar.attn_decode_weight_term(Tk, v_all)
    c.dev = tuple(t.cuda() for t in (q, kpc, vpc, ksc, vsc))
    c.fn = ops.attention_decode_shared if form == "bf16" else ops.attention_decode_shared_kv8
    c.S, c.n, c.H, c.group = S, n, H, group
    return c


def run(c, n=None, tk_dev=None):
    q, kp, vp, ks, vs = c.dev
    return c.fn(q, kp, vp, c.S, ks, vs, c.H, c.n if n is None else n, c.group, tk_dev=tk_dev)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("form", ["bf16", "e4m3"])
def test_two_launches_against_float64(dev, form, hd, H, Hkv):
    """All seven prefix lengths for the 1-query, the 2-query and the 4-query prefix kernel, with the slice count the dispatcher's rule gives."""
    for S, B, group, n in walk(s_values(form, hd)):
        for fam in ("count", "offset"):
            c = case(form, fam, B, group, S, n, H, Hkv, hd)
            with L.knob("SHARED_SPLIT", slices_of(form, hd, S)):
                verify(dev, c, f"shared 2-launch {form} hd{hd} H{H} Hkv{Hkv} B{B} group{group} S{S} n{n} {fam}", f"decode-shared-{form} o")


@pytest.mark.parametrize("H,Hkv", [(4, 4), (8, 2)])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("form", ["bf16", "e4m3"])
def test_one_launch_against_float64(dev, form, hd, H, Hkv):
    """The one-launch form, as the dispatcher itself picks it for these shapes: S = 1, the joined length S + n + 1 one below, at and one above
    one trip of its 16 waves, the prefix alone around that trip, and two trips + 1; for groups 1, 2 and one of 3, 4, 5, 8."""
    t = trip_of(form, hd, waves=16)
    for i, (S, n) in enumerate([(1, 0), (t - 3, 1), (t - 2, 1), (t - N_SUF + 1, N_SUF - 1), (t - 1, 0), (t, 1), (t + 1, N_SUF - 1), (2 * t, 0)]):
        for j, group in enumerate((1, 2, FOUR[i % len(FOUR)])):
            B = 1 if group == 8 or (i + j) % 2 else 3
            for fam in ("count", "offset"):
                c = case(form, fam, B, group, S, n, H, Hkv, hd)
                what = f"shared 1-launch {form} hd{hd} H{H} Hkv{Hkv} B{B} group{group} S{S} n{n} {fam}"
                o = verify(dev, c, what, f"decode-shared1-{form} o")
                with L.knob("SHARED_SPLIT", -1):
                    assert torch.equal(run(c), o), f"{what}: forced, the one-launch form gives other bits"


def verify(dev, c, what, tag):
    o = run(c)
    check(o, c.o64, c.bar, what, tag)
    # the length from device memory, and a second launch: the same bits
    td = torch.tensor([c.n], device=dev, dtype=torch.int32)
    assert torch.equal(run(c, n=0, tk_dev=td), o), f"{what}: tk_dev differs from the host length"
    assert torch.equal(run(c), o), f"{what}: two launches differ"
    return o


@pytest.mark.parametrize("form", ["bf16", "e4m3"])
def test_dispatcher_picks_two_launches(dev, form):
    """B H = 192 and 17 trips of prefix are more workgroups than the chip holds (at most 8 per CU of 256), so the dispatcher takes the two-launch
    form, and one round of resident workgroups is fewer than the 16 slices the prefix alone would give (at most 10).  The one-launch form,
    forced, at the same shape.  And a forced count that leaves slices empty (S = 5 in 7 slices of 1 row)."""
    B, group, H, Hkv, hd, n = 3, 1, 64, 8, 64, 1
    S = 16 * trip_of(form, hd) + 1
    for fam in ("count", "offset"):
        c = case(form, fam, B, group, S, n, H, Hkv, hd)
        o = run(c)
        check(o, c.o64, c.bar, f"shared {form} B H = 192 S{S} {fam}", f"decode-shared-{form} o")
        with L.knob("SHARED_SPLIT", -1):
            o1 = run(c)
        check(o1, c.o64, c.bar, f"shared 1-launch {form} B H = 192 S{S} {fam}", f"decode-shared1-{form} o")
        c = case(form, fam, 2, 4, 5, 1, 4, 2, 128)
        o = run(c)
        with L.knob("SHARED_SPLIT", 7):
            check(run(c), c.o64, c.bar, f"shared {form} S5 in 7 slices {fam}", f"decode-shared-{form} o")
            if fam == "count":
                assert torch.equal(run(c), o)                    # exact sums: the cut does not show


@pytest.mark.parametrize("group", [2, 3, 4, 8])
@pytest.mark.parametrize("form", ["bf16", "e4m3"])
def test_equal_beams_get_equal_bits(dev, form, group):
    """Two beams of an item with the same q and the same suffix: the same output bits, whichever slots of whichever pass they ride in (the first
    and the last row of item 1; at group 8 they are in different passes)."""
    B, H, Hkv, hd, n = 2, 8, 2, 128, 5
    r0, r1 = group, 2 * group - 1
    c = case(form, "offset", B, group, trip_of(form, hd) + 9, n, H, Hkv, hd, same=(r0, r1))
    for split in (2, -1):                                    # two launches with two slices; one launch
        with L.knob("SHARED_SPLIT", split):
            o = run(c)
        check(o, c.o64, c.bar, f"shared {form} group{group} equal beams, split {split}", f"decode-shared-{form} o")
        assert torch.equal(o[r0], o[r1])
        assert not torch.equal(o[r0], o[r0 - 1])             # another item's beam is another result


@pytest.mark.parametrize("form", ["bf16", "e4m3"])
def test_a_device_length_is_clamped_to_the_suffix_cache(dev, form):
    """n + 1 + *tk_dev beyond N reads the N rows of the suffix cache and nothing after them: the result of n = N - 1, bit for bit."""
    c = case(form, "offset", 2, 3, 40, N_SUF - 1, 4, 2, 64)
    td = torch.tensor([N_SUF + 7], device=dev, dtype=torch.int32)
    for split in (1, -1):                                    # both launch forms
        with L.knob("SHARED_SPLIT", split):
            assert torch.equal(run(c, n=0, tk_dev=td), run(c))


def test_refusals(dev):
    c = case("bf16", "offset", 2, 2, 9, 1, 4, 2, 64)
    q, kp, vp, ks, vs = c.dev
    f = ops.attention_decode_shared
    with pytest.raises(ValueError, match="S=13"):          # beyond the prefix cache (S + 3 = 12 rows)
        f(q, kp, vp, 13, ks, vs, 4, 1, 2)
    with pytest.raises(ValueError, match="S=0"):
        f(q, kp, vp, 0, ks, vs, 4, 1, 2)
    with pytest.raises(ValueError, match="n = 70"):
        f(q, kp, vp, 9, ks, vs, 4, N_SUF, 2)
    with pytest.raises(ValueError, match="group = 3"):
        f(q, kp, vp, 9, ks, vs, 4, 1, 3)
    with pytest.raises(ValueError, match="k_suffix"):
        f(q, kp, vp, 9, ks[:3], vs[:3], 4, 1, 2)
    with pytest.raises(ValueError, match="bf16"):
        f(q.float(), kp, vp, 9, ks, vs, 4, 1, 2)
    with pytest.raises(ValueError, match="head_dim 32"):
        f(q, kp, vp, 9, ks, vs, 8, 1, 2)
    # the C entry: a workspace that is too small, named
    lib = L.load()
    need = lib.avllm_attention_decode_shared_workspace_bytes(4, 4, 64)
    assert need == 4 * 4 * 16 * (64 + 2) * 4                 # 16 slices at the most
    ws = torch.empty(need - 4, dtype=torch.uint8, device=dev)
    o = torch.empty_like(q)
    rc = lib.avllm_attention_decode_shared(L.ptr(q), q.stride(0), L.ptr(kp), L.ptr(vp), 9, kp.shape[1], L.ptr(ks), L.ptr(vs), 2, None, N_SUF, L.ptr(o),
                                           o.stride(0), 4, 2, 4, 64, 0.125, 2, L.ptr(ws), ws.numel(), L.stream_ptr())
    assert rc != 0 and "ws of" in lib.avllm_last_error().decode()
    rc = lib.avllm_attention_decode_shared(L.ptr(q), q.stride(0), L.ptr(kp), L.ptr(vp), 9, kp.shape[1], L.ptr(ks), L.ptr(vs), 2, None, N_SUF, L.ptr(o),
                                           o.stride(0), 4, 3, 4, 64, 0.125, 2, L.ptr(ws), ws.numel(), L.stream_ptr())
    assert rc != 0 and "group=3" in lib.avllm_last_error().decode()
    c8 = case("e4m3", "offset", 2, 2, 9, 1, 4, 2, 64)
    q, kp, vp, ks, vs = c8.dev
    with pytest.raises(ValueError, match="one dtype"):
        ops.attention_decode_shared_kv8(q, c.dev[1], c.dev[2], 9, ks, vs, 4, 1, 2)
