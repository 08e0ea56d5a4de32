"""CPU: which kernel avllm_attention_fwd / avllm_attention_bwd give a call (avllm_attention_plan: pure host code, no device), the ATTN_SHORT knob,
and the two predicates derived from the plan (avllm_attention_fwd_mxq_ok, avllm_attention_bwd_fuses_rope).

The expected kernels were derived by hand from the conditions of av_attention_fwd / av_attention_bwd as they stood before the choice became a
function of its own.  The geometry table of tests/test_attention_pin_gpu.py names a kernel in every test id: here each entry must plan it."""
import ctypes as C

import pytest

import refs64_attention as A
from avllm import lib as L

ERR_ARG = 1
DT = {"bf16": L.BF16, "f32": L.F32}
SHORT = ("short13x7", "short17x9")
MFMA = ("mfma64x4", "mfma128x4")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return L.load()


def plan(lib, B, Tq, Tk, H, hd, causal, dtype=L.BF16, impl=0, kv_heads=0):
    """(forward, backward) kernel names; backward None where the plan gives -1."""
    f, b = L.i32(-7), L.i32(-7)
    assert lib.avllm_attention_plan(B, Tq, Tk, H, hd, int(causal), dtype, impl, kv_heads, C.byref(f), C.byref(b)) == 0, lib.avllm_last_error()
    assert 0 <= f.value < len(L.ATTN_FORMS) and -1 <= b.value < len(L.ATTN_FORMS)
    return L.ATTN_FORMS[f.value], (None if b.value < 0 else L.ATTN_FORMS[b.value])


def fwd(lib, T, hd=64, causal=False, B=2, Tk=None, **kw):
    return plan(lib, B, T, T if Tk is None else Tk, 2, hd, causal, **kw)[0]


@pytest.mark.parametrize("g", A.GEOMETRIES, ids=A.geo_id)
def test_every_pinned_geometry_plans_the_kernel_its_id_names(lib, g):
    want = A.kernel_of(g)
    with L.knob("ATTN_SHORT", 0 if g.knob else 1):
        f, b = plan(lib, g.B, g.Tq, g.Tk, g.H, g.hd, g.causal, DT[g.dt], g.impl, g.Hkv)
    assert f == want, (A.geo_id(g), f)
    # the backward has no short form: those lengths run on the 64-key-tile kernels; everything else keeps the forward's family
    assert b == (None if g.Tq != g.Tk else "mfma64x4" if want in SHORT else want), (A.geo_id(g), b)


def test_kernel_of_strips_the_decorations():
    g = A._g
    assert [A.kernel_of(x) for x in (g("gqa-short13x7", 50, 64, False, "short"), g("tqtk-mfma128x4", 50, 128, False, "mfma", Tk=197),
                                     g("ref-impl1", 70, 64, True, "ref", impl=1), g("ref-f32", 65, 128, True, "ref", dt="f32"),
                                     g("rope-bwd-mfma64x4", 70, 64, True, "mfma"))] == ["short13x7", "mfma128x4", "ref", "ref", "mfma64x4"]
    assert {A.kernel_of(x) for x in A.GEOMETRIES} == set(L.ATTN_FORMS)           # the table reaches every form there is


def test_length_boundaries_of_the_short_forms(lib):
    with L.knob("ATTN_SHORT", 1):
        assert [fwd(lib, T) for T in (1, 208, 209, 272, 273, 1500)] == ["short13x7", "short13x7", "short17x9", "short17x9", "mfma64x4", "mfma64x4"]
        assert [fwd(lib, 197, B=B) for B in (65535, 65536)] == ["short13x7", "mfma64x4"]          # one workgroup per item on grid.y
        assert fwd(lib, 197, Tk=198) == "mfma64x4" and fwd(lib, 150, Tk=200) == "mfma64x4"       # self-attention only


def test_what_never_plans_a_short_form(lib):
    with L.knob("ATTN_SHORT", 1):
        for T in (1, 197, 208, 257, 272):
            assert fwd(lib, T, causal=True) == "mfma64x4"
            assert fwd(lib, T, hd=128) == "mfma128x4" and fwd(lib, T, hd=128, causal=True) == "mfma128x4"
            for hd in (8, 32, 96, 256, 512):
                assert fwd(lib, T, hd=hd) == "ref"
            for hd in (64, 128):
                assert fwd(lib, T, hd=hd, dtype=L.F32) == "ref" and fwd(lib, T, hd=hd, impl=1) == "ref"


def test_the_knob_gives_short_lengths_to_the_general_kernel(lib):
    with L.knob("ATTN_SHORT", 0):
        for T in (1, 16, 197, 208, 209, 257, 272, 273):
            assert fwd(lib, T) == "mfma64x4"
            assert not lib.avllm_attention_fwd_mxq_ok(2, T, 2, 64, L.BF16, 2)
    with L.knob("ATTN_SHORT", 1):
        assert fwd(lib, 197) == "short13x7"


def test_backward_form(lib):
    for hd, dtype, impl, want in ((64, L.BF16, 0, "mfma64x4"), (128, L.BF16, 0, "mfma128x4"), (64, L.BF16, 1, "ref"), (128, L.F32, 0, "ref"),
                                  (32, L.BF16, 0, "ref"), (96, L.BF16, 0, "ref")):
        for causal in (False, True):
            for T in (1, 197, 300):
                assert plan(lib, 2, T, T, 4, hd, causal, dtype, impl, 2)[1] == want
            assert plan(lib, 2, 50, 197, 4, hd, False, dtype, impl, 2)[1] is None       # Tq != Tk: no backward
            assert plan(lib, 2, 33, 130, 4, hd, True, dtype, impl, 2)[1] is None


def test_the_backward_fuses_rope_exactly_on_the_mfma_forms(lib):
    for hd in (32, 64, 96, 128, 512):
        for dtype in (L.BF16, L.F32):
            for impl in (0, 1):
                b = plan(lib, 2, 70, 70, 4, hd, True, dtype, impl, 2)[1]
                assert bool(lib.avllm_attention_bwd_fuses_rope(dtype, hd, impl)) == (b in MFMA), (hd, dtype, impl, b)


def test_mxq_ok_exactly_on_the_short_forms_without_grouped_queries(lib):
    with L.knob("ATTN_SHORT", 1), L.knob("F8_UNFUSED_QUANT", 0):
        for B in (2, 65535, 65536):
            for T in (1, 197, 208, 209, 272, 273, 1500):
                for H, hd in ((2, 64), (3, 64), (12, 64), (1, 128), (2, 128), (4, 32)):
                    for dtype in (L.BF16, L.F32):
                        for kv in (0, H, 1):
                            f = plan(lib, B, T, T, H, hd, False, dtype, 0, kv)[0]
                            want = f in SHORT and (H * hd) % 128 == 0 and kv in (0, H)
                            assert bool(lib.avllm_attention_fwd_mxq_ok(B, T, H, hd, dtype, kv)) == want, (B, T, H, hd, dtype, kv, f)


def test_plan_reports_argument_errors(lib):
    f, b = L.i32(), L.i32()
    for args in ((0, 64, 64, 2), (2, 0, 64, 2), (2, 64, 0, 2), (2, 64, 64, 0)):
        assert lib.avllm_attention_plan(*args, 64, 0, L.BF16, 0, 0, C.byref(f), C.byref(b)) == ERR_ARG
    assert lib.avllm_attention_plan(2, 64, 64, 4, 64, 0, L.BF16, 0, 3, C.byref(f), C.byref(b)) == ERR_ARG
    assert b"not a multiple" in lib.avllm_last_error()
    assert lib.avllm_attention_plan(2, 64, 64, 4, 64, 0, L.BF16, 0, 0, None, C.byref(b)) == ERR_ARG
