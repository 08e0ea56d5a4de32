"""The two encoder forwards (csrc/engine.hip avllm_whisper_encoder_fwd, avllm_clip_vision_cls_fwd) on every case of tests/encoder_cases.py:
geometry x mels x n_ctx x B x layers x precision x knob for Whisper, width x patch grid x N x layers x precision x frame dtype x chunk_frames x
eps x knob for CLIP, against the float64 restatements of tests/refs64_encoders.py.  tests/test_encoder_cases_cpu.py shows on the host that each
list holds every pair of levels, that the reference is the oracle's and the golden fixtures' arithmetic, that a correct bf16 engine has half
of every row's bar to itself and that an encoder with one feature wrong misses the bars.

Per case the C ABI is called the guarded way: the output is a view inside a buffer of a sentinel that must be intact around it, the
workspace is exactly avllm_*_workspace_bytes long, filled with NaN (every byte 0xFF: a NaN as bf16, fp32 and e4m3) and followed by a sentinel
tail that must be intact.  Before the launch the case's forms (the library's predicates under the case's knobs) are held to their
restatement from the sources.  The output is judged by encoder_cases.ratios: every Whisper row / CLIP frame on its own (fp8: every block of
64 rows / frame, against the reference that quantises where the case's forms quantise), and the whole tensor.  CLIP cases then go through
ClipEngine.forward with the case's chunk_frames, in the case's frame dtype, the other one, and the case's again: the first is judged like
the guarded call, the third has the first's bits, and where bf16 holds the frames' values so has the second.

Measured on MI355X, worst row (frame, block) error / bar over the cases of a precision and tower ("The encoders across pairings",
has every case):
  Whisper  bf16 (4 cases with a block) 0.234 .. 0.282, the bf16 stem 0.417 of BF16_ENC_STEM_REL_L2; fp8 (4 with a block) 0.247 .. 0.392, the fp8
           stem 0.002; fp32 (3 with a block) 0.006 .. 0.013, the fp32 stems 0.043 .. 0.224 of F32_ENC_STEM_ABS;
  CLIP     bf16 (5 cases) 0.173 .. 0.255; fp8 (6) 0.020 .. 0.319; fp32 (5) 0.002 .. 0.008.
The whole tensor under the same bar is never above the worst row.  A correct engine uses under 0.3 of a bf16 row's bar and under 0.4 of an
fp8 unit's.  37 tests, 7 s with their float64 references (the slowest, whisper-tiny at 2 x 1500 rows, 0.9 s)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import encoder_cases as EC  # noqa: E402

GUARD = 256                      # sentinel elements before and after the output
TAIL = 4096                      # sentinel bytes after the workspace
SENTINEL, TAIL_BYTE = 777.0, 0xA5


def build(dev, c, chunk=0):
    from avllm.engine import ClipEngine, WhisperEngine
    kw = dict(dtype=EC.engine_dtype(c), device=dev, fp8=c.precision == "fp8")
    if c.tower == "whisper":
        return WhisperEngine(EC.weights(c), EC.cfg_of(c), **kw)
    return ClipEngine(EC.weights(c), EC.cfg_of(c), chunk_frames=chunk, **kw)


def frames_of(dev, c, dtype=None):
    """The case's input on the device: the mel in fp32, the frames in the case's frame dtype (or `dtype`)."""
    x = EC.inputs(c)
    if c.tower == "whisper":
        return x.to(dev)
    return x.to(dev, dtype or (torch.bfloat16 if c.frames == "bf16" else torch.float32))


def guarded_call(dev, eng, c, x, expect_error=None):
    """One call of the C entry point with a NaN workspace of exactly the size the library asks for and a guarded output -> the output [items
    (, tokens), d] on the host."""
    from avllm import lib as L
    lib = L.load()
    items = x.shape[0]
    rows = items * (c.n_ctx if c.tower == "whisper" else 1)
    size_fn, fwd = (lib.avllm_whisper_workspace_bytes, lib.avllm_whisper_encoder_fwd) if c.tower == "whisper" else \
        (lib.avllm_clip_workspace_bytes, lib.avllm_clip_vision_cls_fwd)
    n = int(size_fn(C.byref(eng.desc), items))
    ws = torch.empty(n + TAIL, dtype=torch.uint8, device=dev)
    ws[:n] = 0xFF
    ws[n:] = TAIL_BYTE
    buf = torch.full((2 * GUARD + rows * c.d,), SENTINEL, dtype=eng.dtype, device=dev)
    out = buf[GUARD:GUARD + rows * c.d]
    if c.tower == "clip":
        eng.desc.frames_bf16 = int(x.dtype == torch.bfloat16)
    with EC.knobs(c):
        rc = fwd(C.byref(eng.desc), L.ptr(x), items, L.ptr(out), L.ptr(ws), n, L.stream_ptr())
    torch.cuda.synchronize()
    assert bool((ws[n:] == TAIL_BYTE).all()), f"{c.id}: wrote past its workspace of {n} bytes"
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + rows * c.d:] == SENTINEL).all()), f"{c.id}: wrote outside its output"
    if expect_error is not None:
        with pytest.raises(expect_error):
            L.check(rc)
        assert bool((out == SENTINEL).all()), f"{c.id}: a refused call wrote its output"
        return None
    L.check(rc)
    res = out.float().cpu()
    return res.view(items, c.n_ctx, c.d) if c.tower == "whisper" else res.view(items, c.d)


def check_forms(c):
    f = EC.forms(c)
    assert {k: f[k] for k in ("attn", "nq", "att_q", "ff_q")} == EC.restated_forms(c), (c.id, f)
    return f


def judge(c, got, what):
    r = EC.ratios(c, got, EC.reference(c))
    print(f"RATIO {c.id} {what}: error / {EC.bar_of(c)[1]}: {EC.show(r)}")
    assert EC.worst(r) < 1.0, (c.id, what, r)
    return r


@pytest.mark.parametrize("c", EC.WHISPER, ids=lambda c: c.id)
def test_whisper_matrix(dev, c):
    f = check_forms(c)
    eng = build(dev, c)
    x = frames_of(dev, c)
    got = guarded_call(dev, eng, c, x)
    judge(c, got, f"attn={f['attn']} nq={int(f['nq'])} att_q={int(f['att_q'])} ff_q={int(f['ff_q'])}")
    again = guarded_call(dev, eng, c, x)
    assert torch.equal(again, got), "a second call on another NaN workspace is another result"


@pytest.mark.parametrize("c", EC.CLIP, ids=lambda c: c.id)
def test_clip_matrix(dev, c):
    f = check_forms(c)
    eng = build(dev, c, chunk=c.chunk_frames)
    x = frames_of(dev, c)
    got = guarded_call(dev, eng, c, x)
    judge(c, got, f"attn={f['attn']} nq={int(f['nq'])} att_q={int(f['att_q'])} ff_q={int(f['ff_q'])} V={4 if f['patch_v4'] else 2 if f['patch_v2'] else 1}")
    # through ClipEngine.forward on the same engine: the case's chunks, the case's frame dtype, the other one, the case's again
    other = torch.float32 if c.frames == "bf16" else torch.bfloat16
    with EC.knobs(c):
        first = eng.forward(x).float().cpu()
        second = eng.forward(frames_of(dev, c, other)).float().cpu()
        third = eng.forward(x).float().cpu()
    judge(c, first, f"forward, chunk_frames={c.chunk_frames}")
    assert torch.equal(third, first), "the frame dtype of the call before changed the result"
    assert bool(torch.isfinite(second).all())
    if c.frames == "bf16":                                       # both dtypes hold the same numbers
        assert torch.equal(second, first), "bf16 frames and the same values as fp32 frames give different results"


@pytest.mark.parametrize("name", ["w08", "w03", "c13", "c02"])
def test_a_regrown_workspace_changes_nothing(dev, name):
    """forward(x), then a larger batch that makes the Workspace allocate a new buffer, then forward(x) again: the same bits."""
    from avllm.engine import Workspace
    c = EC.BY_NAME[name]
    eng = build(dev, c, chunk=0)
    x = frames_of(dev, c)
    with EC.knobs(c):
        first = eng.forward(x).clone()
        gen = Workspace.generation
        big = torch.cat([x, x, x[:1]], 0)
        eng.forward(big)
        assert Workspace.generation > gen, "the larger batch did not regrow the workspace"
        eng.ws.buf.fill_(0xFF)
        second = eng.forward(x)
    torch.cuda.synchronize()
    assert torch.equal(first, second)
    judge(c, first.float().cpu(), "forward before the regrowth")


def test_refusals(dev):
    from avllm import lib as L
    from avllm.engine import ClipEngine, WhisperEngine
    # fp8 at a width that is no multiple of 128
    w = EC.variant(EC.BY_NAME["w08"], precision="fp8")
    assert w.d % 128 == 64
    with pytest.raises((ValueError, L.AvllmError)):
        eng = WhisperEngine(EC.weights(w), EC.cfg_of(w), dtype=torch.bfloat16, device=dev, fp8=True)
        eng.forward(EC.inputs(w).to(dev))
    torch.cuda.synchronize()
    # a mel length other than 2 n_ctx, a wrong mel count
    c = EC.BY_NAME["w08"]
    eng = build(dev, c)
    with pytest.raises(ValueError, match="length"):
        eng.forward(EC.inputs(c)[..., :-2].to(dev))
    with pytest.raises(ValueError):
        eng.forward(EC.inputs(c)[:, :-1].to(dev))
    # a wrong image size
    k = EC.BY_NAME["c13"]
    ce = build(dev, k)
    with pytest.raises(ValueError, match="doesn't match"):
        ce.forward(EC.inputs(k)[..., :-32, :-32].to(dev))
    # CLIP without a block: refused by the engine's constructor and by the entry point (which used to return without writing the output)
    k0 = EC.variant(k, layers=1)
    cfg0 = EC.cfg_of(k0)
    cfg0.layers = 0
    with pytest.raises(ValueError, match="layers=0"):
        ClipEngine(EC.weights(k), cfg0, dtype=EC.engine_dtype(k), device=dev)
    ce.desc.layers = 0
    guarded_call(dev, ce, k, frames_of(dev, k), expect_error=ValueError)
    ce.desc.layers = k.layers
    assert guarded_call(dev, ce, k, frames_of(dev, k)) is not None
