"""The two encoder forwards (csrc/engine.hip avllm_whisper_encoder_fwd, avllm_clip_vision_cls_fwd: the stems and encoder_layers) across pairings
of their forms: one case table per tower, the weights and inputs of a case, the launch forms the library's own predicates select for it, the
float64 run of a case on tests/refs64_encoders.py and the judgement of an output against it.  Pure CPU, everything from seeds:
tests/test_encoder_cases_cpu.py checks the tables, the reference, the bars and the judgement on the host, tests/test_encoder_matrix_gpu.py runs
every case on the engines.

WHISPER and CLIP are explicit lists of 16 cases that hold every pair of levels of every two factors at least once, except the refused pairs
(W_IMPOSSIBLE), and start with the deployed forms.  Width, heads and ffn = 4 x width are those of the named checkpoints; the token counts are
cut down where the float64 reference has to stay under a second.

Whisper levels.  geom: tiny 384 / 6, small 768 / 12, large 1280 / 20 (large-v3), w320 320 / 5 (a multiple of 64, not of 128: fp8 refused).
n_ctx: 1500 (on tiny and w320 only: the issue's rule, a case's float64 reference stays in seconds), 100 (<= 208: SHORT13X7), 231 (209 .. 272:
SHORT17X9; odd, so the 64-column slabs of im2col1 and every 64-row tile end ragged), 300 (> 272 and no multiple of 64: MFMA64X4 with a ragged
last tile).  layers 0 is the stem and the final norm alone, under the tight bars BF16_ENC_STEM_REL_L2 / F32_ENC_STEM_ABS.

CLIP levels.  width: w128 128 / 2, b 768 / 12, l 1024 / 16.  grid: p32 on 224 (50 tokens), p16 on 224 (197), p14 on 224 (257, K 588 -> 640
padded, V = 2), p14-336 (577: MFMA64X4 with a ragged last tile), p7-105 (an odd patch, V = 1, K 147 -> 192 padded, 15 x 15 + 1 = 226 tokens).
Token counts are g * g + 1: 197, 226, 257, 290 for g = 14 .. 17, so no whole-patch image lands on 208 | 209 or 272 | 273; 197 and 226 are the
two sides of the first switch that exist and 257 (SHORT17X9) and 577 (MFMA64X4) those of the second.  N: 1, 3, 5 (5 x tokens is a multiple of
256 for no grid here).  chunk: 0, `div` = 1 frame per call, `nondiv` = 2 (N = 3: 2 + 1, N = 5: 2 + 2 + 1; N = 1: one call either way).

Plants (the last column but one).  "loweps": a LayerNorm input whose variance is of the size of eps, so that eps decides the value -- Whisper:
conv2's weight and bias x 0.01 and the position table x 0.03 (every stem row has variance ~ 1e-5); CLIP: pos[0] = -class_emb + 0.003 N, so the
CLS row of every frame enters pre_layrnorm with variance ~ 1e-5 (only the CLS row reaches the output).  "big": one item's mel x 8 (B = 1: 20
columns of it) / one frame x 16, so that a neighbour's data leaking in would show.  Plants are part of the case: both sides hold the same numbers."""
import contextlib
import ctypes as C
import itertools
from types import SimpleNamespace

import torch

import refs64_encoders as RE

W_GEOM = {"tiny": (384, 6), "small": (768, 12), "large": (1280, 20), "w320": (320, 5)}
C_WIDTH = {"w128": (128, 2), "b": (768, 12), "l": (1024, 16)}
C_GRID = {"p32": (224, 32), "p16": (224, 16), "p14": (224, 14), "p14-336": (336, 14), "p7-105": (105, 7)}
KNOBS = {"none": (), "short0": (("ATTN_SHORT", 0),), "unfused": (("F8_UNFUSED_QUANT", 1),)}

W_FACTORS = {"geom": tuple(W_GEOM), "mels": (80, 128), "n_ctx": (1500, 100, 231, 300), "B": (1, 2, 3), "layers": (0, 1, 2),
             "precision": ("fp32", "bf16", "fp8"), "knob": tuple(KNOBS)}
C_FACTORS = {"width": tuple(C_WIDTH), "grid": tuple(C_GRID), "N": (1, 3, 5), "layers": (1, 2, 3), "precision": ("fp32", "bf16", "fp8"),
             "frames": ("fp32", "bf16"), "chunk": ("0", "div", "nondiv"), "eps": (1e-5, 1e-6), "knob": tuple(KNOBS)}
FACTORS = {"whisper": W_FACTORS, "clip": C_FACTORS}

# the refused pairs, each with the refusing line
W_IMPOSSIBLE = (
    ("geom", "w320", "precision", "fp8"),      # engine.hip avllm_whisper_encoder_fwd: "whisper: fp8 needs bf16 activations and widths that are multiples of 128"
    ("geom", "small", "n_ctx", 1500),          # the issue: 1500 on the narrow widths only (the float64 reference of a case stays in seconds)
    ("geom", "large", "n_ctx", 1500),          # the same
)
C_IMPOSSIBLE = ()                              # every CLIP width here is a multiple of 128
IMPOSSIBLE = {"whisper": W_IMPOSSIBLE, "clip": C_IMPOSSIBLE}

# name, the levels in the order of the factors, plants, seed.  The first rows are the deployed forms (whisper-tiny whole; whisper-small and
# large-v3 at a cut n_ctx; ViT-B/16 with the bf16 frames of the device-side preprocessing, ViT-L/14 in fp8); the next three of each list pin the
# fp8 compositions and knobs (fp8 with F8_UNFUSED_QUANT or ATTN_SHORT = 0 is given blocks to act on); the rest complete the pairs (an annealing search, then written out and adjusted by hand for the forms).
_W_TABLE = (
    ("tiny-whole", "tiny", 80, 1500, 2, 2, "bf16", "none", "", 6100),
    ("small-300", "small", 80, 300, 1, 2, "bf16", "none", "big", 6101),
    ("large-v3-fp8", "large", 128, 300, 3, 1, "fp8", "none", "", 6102),
    ("w03", "small", 80, 100, 2, 1, "fp8", "none", "big", 6103),
    ("w04", "tiny", 128, 231, 3, 2, "fp8", "short0", "", 6104),
    ("w05", "tiny", 80, 1500, 1, 1, "fp8", "unfused", "", 6105),
    ("w06", "w320", 128, 1500, 3, 0, "fp32", "short0", "", 6106),
    ("w07", "tiny", 80, 300, 3, 0, "fp8", "none", "big", 6107),
    ("w08", "w320", 80, 231, 1, 1, "bf16", "none", "loweps", 6108),
    ("w09", "w320", 128, 100, 1, 0, "fp32", "none", "loweps", 6109),
    ("w10", "w320", 80, 300, 2, 2, "fp32", "unfused", "big", 6110),
    ("w11", "small", 128, 231, 3, 0, "bf16", "unfused", "loweps", 6111),
    ("w12", "small", 80, 300, 2, 1, "fp32", "short0", "big", 6112),
    ("w13", "large", 80, 100, 1, 2, "bf16", "short0", "big", 6113),
    ("w14", "tiny", 128, 100, 3, 1, "fp32", "unfused", "loweps", 6114),
    ("w15", "large", 128, 231, 2, 0, "fp32", "unfused", "", 6115),
)
_C_TABLE = (
    ("vit-b16", "b", "p16", 3, 2, "bf16", "bf16", "0", 1e-5, "none", "big", 6200),
    ("vit-l14-fp8", "l", "p14", 3, 2, "fp8", "fp32", "0", 1e-5, "none", "", 6201),
    ("c02", "w128", "p16", 5, 2, "fp8", "bf16", "div", 1e-6, "none", "big", 6202),
    ("c03", "b", "p7-105", 3, 3, "fp8", "fp32", "nondiv", 1e-5, "short0", "", 6203),
    ("c04", "b", "p32", 5, 2, "fp8", "bf16", "div", 1e-6, "unfused", "big", 6204),
    ("c05", "w128", "p16", 1, 1, "fp8", "fp32", "div", 1e-5, "short0", "", 6205),
    ("c06", "l", "p32", 1, 3, "fp32", "fp32", "0", 1e-6, "short0", "loweps", 6206),
    ("c07", "w128", "p7-105", 1, 2, "fp32", "bf16", "div", 1e-6, "none", "", 6207),
    ("c08", "l", "p14-336", 3, 1, "fp32", "fp32", "div", 1e-5, "unfused", "big", 6208),
    ("c09", "l", "p7-105", 5, 1, "bf16", "bf16", "0", 1e-5, "unfused", "big", 6209),
    ("c10", "b", "p14-336", 1, 2, "bf16", "bf16", "nondiv", 1e-6, "short0", "loweps", 6210),
    ("c11", "w128", "p14-336", 5, 3, "fp8", "fp32", "0", 1e-6, "none", "", 6211),
    ("c12", "w128", "p14", 1, 3, "bf16", "fp32", "div", 1e-5, "unfused", "loweps", 6212),
    ("c13", "w128", "p32", 3, 1, "bf16", "bf16", "nondiv", 1e-5, "none", "loweps", 6213),
    ("c14", "l", "p16", 3, 3, "fp32", "bf16", "nondiv", 1e-6, "unfused", "loweps", 6214),
    ("c15", "b", "p14", 5, 1, "fp32", "bf16", "nondiv", 1e-6, "short0", "big", 6215),
)


def _case(tower, name, *rest):
    *levels, plants, seed = rest
    F = FACTORS[tower]
    c = SimpleNamespace(tower=tower, name=name, seed=seed, plants=tuple(p for p in plants.split("+") if p), **dict(zip(F, levels)))
    if tower == "whisper":
        c.d, c.heads = W_GEOM[c.geom]
        c.items, c.tokens = c.B, c.n_ctx
    else:
        c.d, c.heads = C_WIDTH[c.width]
        c.image, c.patch = C_GRID[c.grid]
        c.items, c.tokens = c.N, (c.image // c.patch) ** 2 + 1
        c.chunk_frames = {"0": 0, "div": 1, "nondiv": 2}[c.chunk]
    c.ffn = 4 * c.d
    c.id = "-".join([name] + [str(v) for v in levels] + list(c.plants))
    return c


WHISPER = [_case("whisper", *row) for row in _W_TABLE]
CLIP = [_case("clip", *row) for row in _C_TABLE]
CASES = {"whisper": WHISPER, "clip": CLIP}
BY_NAME = {c.name: c for c in WHISPER + CLIP}


def levels_of(c):
    return {f: getattr(c, f) for f in FACTORS[c.tower]}


def variant(c, seed=None, **levels):
    """Case c with some levels (or its seed) changed."""
    lv = dict(levels_of(c), **levels)
    tag = "~".join([c.name] + [f"{k}={v}" for k, v in levels.items()] + ([f"seed={seed}"] if seed is not None else []))
    return _case(c.tower, tag, *[lv[f] for f in FACTORS[c.tower]], "+".join(c.plants), c.seed if seed is None else seed)


def missing_pairs(tower, cases=None):
    """The (factor, level, factor, level) pairs no case of the tower's list holds, the IMPOSSIBLE ones left out."""
    F = FACTORS[tower]
    want = {(fa, a, fb, b) for fa, fb in itertools.combinations(F, 2) for a in F[fa] for b in F[fb]} - set(IMPOSSIBLE[tower])
    for c in CASES[tower] if cases is None else cases:
        lv = levels_of(c)
        want -= {(fa, lv[fa], fb, lv[fb]) for fa, fb in itertools.combinations(F, 2)}
    return sorted(want, key=str)


# ---------------------------------------------------------------- a case's model and inputs
def engine_dtype(c):
    return torch.float32 if c.precision == "fp32" else torch.bfloat16


def cfg_of(c):
    from avllm.arch import ClipCfg, WhisperCfg
    if c.tower == "whisper":
        return WhisperCfg(c.d, c.heads, c.layers, c.ffn, c.mels, c.n_ctx)
    return ClipCfg(c.d, c.heads, c.layers, c.ffn, c.image, c.patch, c.eps)


_WEIGHTS, _INPUTS = {}, {}


def weights(c):
    """The HF-named state dict of case c, drawn as avllm.arch.synth_whisper / synth_clip draw it in the engine dtype and held as float32 (the
    engine and the reference hold the same numbers), then the "loweps" plant.  Cached."""
    if c.name in _WEIGHTS:
        return _WEIGHTS[c.name]
    from avllm import arch
    dt = engine_dtype(c)
    sd = (arch.synth_whisper if c.tower == "whisper" else arch.synth_clip)(cfg_of(c), "cpu", dt, c.seed)
    sd = {k: v.float() for k, v in sd.items()}
    if "loweps" in c.plants:
        rd = lambda t: t.to(dt).float()                                          # noqa: E731
        if c.tower == "whisper":
            sd["encoder.conv2.weight"], sd["encoder.conv2.bias"] = rd(sd["encoder.conv2.weight"] * 0.01), rd(sd["encoder.conv2.bias"] * 0.01)
            sd["encoder.embed_positions.weight"] = rd(sd["encoder.embed_positions.weight"] * 0.03)
        else:
            g = torch.Generator().manual_seed(40000 + c.seed)
            pos = sd["embeddings.position_embedding.weight"].clone()
            pos[0] = rd(-sd["embeddings.class_embedding"] + 0.003 * torch.randn(c.d, generator=g))
            sd["embeddings.position_embedding.weight"] = pos
    _WEIGHTS[c.name] = sd
    return sd


def inputs(c):
    """randn mel [B, mels, 2 n_ctx] / frames [N, 3, S, S] as float32 tensors whose values the engine dtype holds (bf16 frames: bf16 holds them
    whatever the engine), then the "big" plant.  Cached."""
    if c.name in _INPUTS:
        return _INPUTS[c.name]
    g = torch.Generator().manual_seed(9000 + c.seed)
    if c.tower == "whisper":
        x = torch.randn(c.B, c.mels, 2 * c.n_ctx, generator=g)
        if "big" in c.plants:
            if c.B > 1:
                x[1] *= 8.0
            else:
                x[0, :, c.n_ctx:c.n_ctx + 20] *= 8.0
        dt = engine_dtype(c)
    else:
        x = torch.randn(c.N, 3, c.image, c.image, generator=g)
        if "big" in c.plants:
            x[min(1, c.N - 1)] *= 16.0
        dt = torch.bfloat16 if c.frames == "bf16" else engine_dtype(c)
    _INPUTS[c.name] = x.to(dt).float()
    return _INPUTS[c.name]


# ---------------------------------------------------------------- the launch forms of a case
@contextlib.contextmanager
def knobs(c):
    """The library's A/B switches of case c for the duration of the block."""
    from avllm import lib as L
    with contextlib.ExitStack() as st:
        for name, value in KNOBS[c.knob]:
            st.enter_context(L.knob(name, value))
        yield


def _knob_value(name):
    from avllm import lib as L
    v = L.i32()
    L.check(L.load().avllm_get_knob(name.encode(), C.byref(v)))
    return v.value


def forms(c):
    """Which launch forms case c takes, from the library's own predicates under the case's knobs (host code only: nothing here touches a GPU):
    avllm_attention_plan, avllm_attention_fwd_mxq_ok, avllm_gemm_f8_takes_quantised_output, and the two conditions engine.hip does not export,
    restated with their lines -- nq (encoder_layers: fp8 && d % 128 == 0 && d <= 8192 && !F8_UNFUSED_QUANT) and the patchify V
    (elementwise.hip av_clip_patchify: p % 4 == 0 ? 4 : p % 2 == 0 ? 2 : 1).  att_q and ff_q exist in the blocks that are not CLIP's CLS-only
    last one; "attn" is None without a block."""
    from avllm import lib as L
    from avllm import ops
    lib = L.load()
    fp8 = c.precision == "fp8"
    dt = L.F32 if c.precision == "fp32" else L.BF16
    hd = c.d // c.heads
    full_blocks = c.layers if c.tower == "whisper" else c.layers - 1
    with knobs(c):
        unfused = _knob_value("F8_UNFUSED_QUANT") != 0
        attn = ops.attention_plan(c.items, c.tokens, c.tokens, c.heads, hd, False, dt)[0] if c.layers else None
        nq = fp8 and c.layers > 0 and c.d % 128 == 0 and c.d <= 8192 and not unfused
        att_q = fp8 and full_blocks > 0 and bool(lib.avllm_attention_fwd_mxq_ok(c.items, c.tokens, c.heads, hd, dt, c.heads))
        M = c.items * c.tokens
        q1 = L.GemmF8Desc()                                      # fc1 as encoder_layers describes it; the pointers are only tested for alignment
        q1.A, q1.SA, q1.B, q1.SB, q1.bias, q1.Cq, q1.SCq = (4096,) * 7
        q1.lda, q1.ldb, q1.M, q1.N, q1.K, q1.act, q1.ldcq = c.d, c.d, M, c.ffn, c.d, 1, c.ffn
        ff_q = fp8 and full_blocks > 0 and not unfused and bool(lib.avllm_gemm_f8_takes_quantised_output(C.byref(q1)))
    out = {"attn": attn, "nq": nq, "att_q": att_q, "ff_q": ff_q}
    for name in ("ref", "short13x7", "short17x9", "mfma64x4"):
        out["attn_" + name] = attn == name
    if c.tower == "whisper":
        out["k_padded"] = (3 * c.mels) % 64 != 0
    else:
        out["k_padded"] = (3 * c.patch * c.patch) % 64 != 0
        v = 4 if c.patch % 4 == 0 else 2 if c.patch % 2 == 0 else 1
        out.update(patch_v4=v == 4, patch_v2=v == 2, patch_v1=v == 1, frames_bf16=c.frames == "bf16",
                   chunked=0 < c.chunk_frames < c.N, ragged_chunk=0 < c.chunk_frames < c.N and c.N % c.chunk_frames != 0)
    return out


def restated_forms(c):
    """forms(c) restated from the sources, for the checks to hold the predicates to: csrc/attention.hip av_attention_fwd_form (fp32 -> ref;
    head dim 64, non-causal, Tq == Tk: <= 208 SHORT13X7, <= 272 SHORT17X9 unless ATTN_SHORT = 0, else MFMA64X4) and av_attention_fwd_mxq_ok
    (a short form, d % 128 == 0, !F8_UNFUSED_QUANT); csrc/engine.hip encoder_layers (nq; att_q and the quantised fc1 output only in blocks
    that are not CLIP's CLS-only last one); csrc/fp8_fast.hip f8_fast_takes (M > 128, at least 64 tiles of 256 x 256, K >= 256, N % 128 == 0)."""
    fp8, unfused = c.precision == "fp8", c.knob == "unfused"
    full_blocks = c.layers if c.tower == "whisper" else c.layers - 1
    assert c.d // c.heads == 64
    if not c.layers:
        attn = None
    elif c.precision == "fp32":
        attn = "ref"
    elif c.knob != "short0" and c.tokens <= 208:
        attn = "short13x7"
    elif c.knob != "short0" and c.tokens <= 272:
        attn = "short17x9"
    else:
        attn = "mfma64x4"
    M = c.items * c.tokens
    tiles = -(-M // 256) * -(-c.ffn // 256)
    return {"attn": attn, "nq": fp8 and c.layers > 0 and c.d % 128 == 0 and not unfused,
            "att_q": fp8 and full_blocks > 0 and attn in ("short13x7", "short17x9") and c.d % 128 == 0 and not unfused,
            "ff_q": fp8 and full_blocks > 0 and not unfused and M > 128 and tiles >= 64 and c.d >= 256 and c.ffn % 128 == 0}


BOOLEAN_FORMS = {"whisper": ("nq", "att_q", "ff_q", "attn_ref", "attn_short13x7", "attn_short17x9", "attn_mfma64x4", "k_padded"),
                 "clip": ("nq", "att_q", "ff_q", "attn_ref", "attn_short13x7", "attn_short17x9", "attn_mfma64x4", "k_padded", "patch_v4", "patch_v2",
                          "patch_v1", "frames_bf16", "chunked", "ragged_chunk")}


def fp8_of(c, f=None):
    """The fp8= of the reference that reads each quantiser's input where case c's forms read it (None outside fp8)."""
    if c.precision != "fp8":
        return None
    f = forms(c) if f is None else f
    return {k: f[k] for k in ("nq", "att_q", "ff_q")}


# ---------------------------------------------------------------- the float64 run of a case
_REF = {}


def run_ref(c, **kw):
    fn = RE.whisper if c.tower == "whisper" else RE.clip_cls
    if c.tower == "clip":
        kw.setdefault("chunk", c.chunk_frames)
    with torch.no_grad():
        return fn(weights(c), cfg_of(c), inputs(c), **kw)


def reference(c):
    """The float64 output the engine's is judged against, computed once per case and left unchanged: the plain reference (fp32, bf16) or its
    fp8 form with the case's forms."""
    if c.name not in _REF:
        _REF[c.name] = run_ref(c, fp8=fp8_of(c))
    return _REF[c.name]


# ---------------------------------------------------------------- the judgement
FP8_BLOCK_ROWS = 64


def bar_of(c):
    """(the bar, its name in tests/bars.py) of case c's rows."""
    import bars as Bar
    stem = c.tower == "whisper" and c.layers == 0
    if c.precision == "fp32":
        return (Bar.F32_ENC_STEM_ABS, "F32_ENC_STEM_ABS") if stem else (Bar.F32_LOGITS_ABS, "F32_LOGITS_ABS")
    if c.precision == "bf16":
        return (Bar.BF16_ENC_STEM_REL_L2, "BF16_ENC_STEM_REL_L2") if stem else (Bar.BF16_ENC_REL_L2, "BF16_ENC_REL_L2")
    return Bar.FP8_ENC_UNIT_REL_L2, "FP8_ENC_UNIT_REL_L2"


def units(c, t):
    """t as [units, n]: what is judged on its own.  Whisper: every output row [d] (fp8: every block of 64 rows of an item, the last one
    ragged, padded here with zeros); CLIP: every frame's CLS row.  No row is left out."""
    t = t.detach().to("cpu").to(torch.float64)
    if c.tower == "clip":
        return t.reshape(c.N, c.d)
    t = t.reshape(c.B, c.n_ctx, c.d)
    if c.precision != "fp8":
        return t.reshape(c.B * c.n_ctx, c.d)
    nb = -(-c.n_ctx // FP8_BLOCK_ROWS)
    pad = torch.zeros(c.B, nb * FP8_BLOCK_ROWS, c.d, dtype=torch.float64)
    pad[:, :c.n_ctx] = t
    return pad.reshape(c.B * nb, FP8_BLOCK_ROWS * c.d)


def unit_errors(c, got, ref):
    """Per unit: max |error| (fp32) or the relative L2 error (bf16, fp8).  A unit with a non-finite value is infinitely wrong."""
    g, r = units(c, got), units(c, ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    if c.precision == "fp32":
        e = (g - r).abs().amax(1)
    else:
        e = (g - r).norm(dim=1) / r.norm(dim=1).clamp_min(1e-300)
    return torch.where(torch.isfinite(g).all(1) & torch.isfinite(e), e, torch.full_like(e, float("inf")))


def ratios(c, got, ref):
    """The checked quantities of an encoder output as error / bar: "rows" (the worst unit of units()), "tensor" (the whole output under the
    same bar: what the suite asserted before), and the index of the worst unit."""
    bar, _ = bar_of(c)
    e = unit_errors(c, got, ref)
    g, r = got.detach().to("cpu").to(torch.float64).flatten(), ref.to(torch.float64).flatten()
    whole = float((g - r).abs().max()) if c.precision == "fp32" else float((g - r).norm() / r.norm())
    if not bool(torch.isfinite(g).all()):
        whole = float("inf")
    return {"rows": float(e.max()) / bar, "tensor": whole / bar, "worst unit": int(e.argmax())}


def worst(ratio):
    return max(ratio["rows"], ratio["tensor"])


def show(ratio):
    return f"rows {ratio['rows']:.3f} tensor {ratio['tensor']:.3f} (worst unit {ratio['worst unit']})"
