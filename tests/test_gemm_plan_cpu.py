"""CPU: which kernel avllm_gemm gives a call (avllm_gemm_plan: pure host code, no device), the GEMM_VARIANT knob and lib.knob's restore.

The expected kernels were derived by hand from the conditions of av_gemm as it stood before the choice became a function of its own; the
thresholds behind them are measurements (DESIGN.md "Which GEMM kernel a call gets"), so a slip in one costs speed, not correctness, and
no numerical test can see it."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from avllm import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED = 1, 4
A_, B_, C_, A2_, B2_, BIAS_, R_ = (0x100000 * (i + 1) for i in range(7))      # fake operands: non-null, 16-byte aligned, never read


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return L.load()


def desc(M, N, K, K2=0, dtype=L.BF16, **kw):
    d = L.GemmDesc()
    d.A, d.B, d.C, d.lda, d.ldb, d.ldc = A_, B_, C_, K, K, N
    d.M, d.N, d.K, d.dtype, d.alpha = M, N, K, dtype, 1.0
    if K2:
        d.A2, d.B2, d.lda2, d.ldb2, d.K2 = A2_, B2_, K2, K2, K2
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


def plan(lib, d):
    """(rc, kernel name)"""
    k = L.i32(-1)
    rc = lib.avllm_gemm_plan(C.byref(d), C.byref(k))
    return rc, (L.GEMM_KERNELS[k.value] if rc == 0 else None)


TILINGS_CALL = dict(M=700, N=520, K=256, K2=64, bias=BIAS_, R=R_, ldr=520, act=L.ACT_GELU)      # the call of test_every_gemm_tiling_agrees
HUGE = (6000000, 2304, 768)                                                                     # M * lda >= 4e9: past 32-bit row offsets

AUTO = [
    (desc(4096, 4096, 4096), "WP4"),
    (desc(4096, 12288, 4096, K2=192), "WP4"),
    (desc(4096, 4096, 4096, out_f32=1), "W4"),
    (desc(4096, 4096, 2048, out_f32=1), "H16"),
    (desc(8192, 8192, 2048, out_f32=1), "W4"),                       # 1024 tiles
    (desc(394000, 768, 768, R=R_, ldr=768, r_mod=9), "H16"),         # broadcast residual rows
    (desc(394000, 768, 768), "WP4"),
    (desc(4096, 4096, 4096, alpha=0.5), "W4"),
    (desc(4096, 4096, 4096, C=C_ + 8), "W4"),                        # not lean: C off 16 bytes
    (desc(2048, 2048, 16384), "RING"),
    (desc(2048, 2048, 4096), "128"),
    (desc(128, 65536, 4096), "128"),                                 # M > 128 fails
    (desc(*HUGE), "128"),                                            # fails fits32
    (desc(16, 4096, 4096), "SMALLM"),
    (desc(16, 4096, 320), "128"),                                    # K % 256 != 0
    (desc(16, 4096, 4096, drop_p=0.1), "128"),
    (desc(4096, 64, 4096), "SKINNY64"),
    (desc(100, 64, 4096), "128"),
    (desc(100, 64, 4096, a_drop_p=0.1), "SKINNY64"),
    (desc(4096, 4096, 4096, dtype=L.F32), "F32"),
]


@pytest.mark.parametrize("i", range(len(AUTO)))
def test_automatic_choice(lib, i):
    d, want = AUTO[i]
    with L.knob("GEMM_VARIANT", 0):
        assert plan(lib, d) == (0, want), (d.M, d.N, d.K, d.K2)


def test_a_drop_outside_the_rank_side_kernel_is_unsupported(lib):
    with L.knob("GEMM_VARIANT", 0):
        assert plan(lib, desc(4096, 4096, 4096, a_drop_p=0.1))[0] == ERR_UNSUPPORTED
        assert b"a_drop_p" in lib.avllm_last_error()


FORCED = [(v, desc(**TILINGS_CALL), k) for v, k in ((1, "128"), (2, "RING"), (5, "H16"), (6, "HP16"), (7, "W4"), (8, "WP4"), (9, "DP"))] + [
    (8, desc(4096, 4096, 4096, out_f32=1), "128"),                   # a variant that cannot take the call: 128x128, not the automatic choice
    (7, desc(4096, 4096, 64), "128"),
    (9, desc(128, 4096, 4096), "128"),
    (1, desc(16, 4096, 4096), "128"),                                # a forced variant switches the small-M kernel off
    (6, desc(*HUGE), "HP16"),
    (1, desc(4096, 64, 4096), "SKINNY64"),
]


@pytest.mark.parametrize("i", range(len(FORCED)))
def test_forced_variant(lib, i):
    v, d, want = FORCED[i]
    with L.knob("GEMM_VARIANT", v):
        assert plan(lib, d) == (0, want), (v, d.M, d.N, d.K, d.K2)


def test_forced_16wave_kernel_refuses_operands_past_32bit_offsets(lib):
    with L.knob("GEMM_VARIANT", 5):
        assert plan(lib, desc(*HUGE))[0] == ERR_ARG
        assert b"32-bit row offsets" in lib.avllm_last_error()


def test_plan_reports_the_argument_errors_of_gemm(lib):
    for d in (desc(4096, 4096, 4096, A=None), desc(0, 4096, 4096), desc(4096, 4096, 96), desc(4096, 4096, 4096, lda=4100),
              desc(4096, 4096, 4096, dtype=7), desc(4096, 64, 4096, n_valid=65), desc(100, 64, 4096, a_drop_p=0.1, lda=8192)):
        assert plan(lib, d)[0] == ERR_ARG
    d = desc(4096, 4096, 4096, K2=64)
    d.A2 = None
    assert plan(lib, d)[0] == ERR_ARG


def test_nonpositive_variant_is_automatic(lib):
    with L.knob("GEMM_VARIANT", -1):
        assert plan(lib, desc(16, 4096, 4096)) == (0, "SMALLM")
        assert plan(lib, desc(4096, 4096, 4096)) == (0, "WP4")


def get(lib, name):
    v = L.i32()
    L.check(lib.avllm_get_knob(name.encode(), C.byref(v)))
    return v.value


def test_knob_restores_what_it_found(lib):
    before = get(lib, "GEMM_GW")
    with L.knob("GEMM_GW", 3):                                       # a value that is neither the default nor the environment's
        with L.knob("GEMM_GW", 6):
            assert get(lib, "GEMM_GW") == 6
        assert get(lib, "GEMM_GW") == 3                              # nested
        with pytest.raises(ZeroDivisionError), L.knob("GEMM_GW", 5):
            assert get(lib, "GEMM_GW") == 5
            1 / 0
        assert get(lib, "GEMM_GW") == 3                              # after an exception in the block
    assert get(lib, "GEMM_GW") == before


def test_unknown_knob_is_an_error(lib):
    v = L.i32()
    assert lib.avllm_get_knob(b"NO_SUCH_KNOB", C.byref(v)) == ERR_ARG
    assert lib.avllm_set_knob(b"NO_SUCH_KNOB", 1) == ERR_ARG
    with pytest.raises(ValueError), L.knob("NO_SUCH_KNOB", 1):
        pass


def test_environment_variant_holds_from_the_first_call(lib):
    """AVLLM_GEMM_VARIANT in the environment of a fresh process: the very first call, an M = 16 one, is already off the small-M kernel
    (the switch used to be read by the first tiled call only, so the same call got a different kernel depending on what ran before it)."""
    code = ("import ctypes as C\nfrom avllm import lib as L\nd = L.GemmDesc()\n"
            "d.A, d.B, d.C, d.lda, d.ldb, d.ldc, d.M, d.N, d.K, d.dtype, d.alpha = 4096, 8192, 12288, 4096, 4096, 4096, 16, 4096, 4096, L.BF16, 1.0\n"
            "k = L.i32(-1)\nassert L.load().avllm_gemm_plan(C.byref(d), C.byref(k)) == 0\nprint('kernel', L.GEMM_KERNELS[k.value])\n")
    env = dict(os.environ, AVLLM_GEMM_VARIANT="5", PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "audio-visual-llm_amd"), os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "kernel 128" in out.stdout, out.stdout
    env.pop("AVLLM_GEMM_VARIANT")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert "kernel SMALLM" in out.stdout, out.stdout + out.stderr
