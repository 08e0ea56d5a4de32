"""generate(share_prefix=True) on the tiny golden model (tests/golden/g2_tiny_e2e.npz): the beams of an item, or its sampled sequences, read one
prefix cache (the B-row cache of the prefill) and keep their generated positions in a suffix cache (LlamaEngine.decode_step_shared,
csrc/attention_decode_shared.hip).

Step level: the same tokens forced through decode_step on a materialised copy cache and through decode_step_shared, with a parent permutation
applied to both between steps.  Beam search: test_generate_beam_gpu.py's teacher-forced rule (and test_generate_kv8_gpu.py's for the fp8 cache).
Sampled n-best: every returned token's log-probability against the teacher-forced one of its row's own history, and a prefill of B rows.
Fallbacks (more than 16 rows, fp32, the fused step off, greedy, n = 1) and the default are bit-equal to share_prefix=False."""
import glob
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import generate_ref  # noqa: E402
import kv8_cases as K  # noqa: E402
import refs64_kv8 as R64  # noqa: E402
from avllm import lib as L  # noqa: E402
from avllm import ops  # noqa: E402
from bars import BF16_LOGIT_MAX_ABS, BF16_LOGITS_REL_L2, rel_l2  # noqa: E402
from generate_ref import with_eos  # noqa: E402
from test_generate_beam_gpu import seq_logprob  # noqa: E402
from test_generate_fp8_gpu import _model  # noqa: E402
from test_model_gpu import make_model, tiny  # noqa: E402,F401

BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NEW = 6


@pytest.fixture(scope="module")
def m16(dev, tiny):  # noqa: F811
    g, oc, W, *_ = tiny
    return make_model(oc, W, "bf16", max_seq_len=256).eval()


def built(**kw):
    """The same golden model (adapters on, max_seq_len 256, bf16) with constructor options."""
    oc, W, _, _ = K.tiny()
    return _model(W, oc, with_lora=True, precision="bf16", **kw)


class Spy:
    """Counts the engine calls of one generate() and notes the rows of its prefill."""

    def __init__(self, eng):
        self.eng, self.shared, self.plain, self.prefill_rows = eng, 0, 0, []
        self.orig = (eng.decode_step_shared, eng.decode_step, eng.prefill)

    def __enter__(self):
        def shared(*a, **k):
            self.shared += 1
            return self.orig[0](*a, **k)

        def plain(*a, **k):
            self.plain += 1
            return self.orig[1](*a, **k)

        def prefill(x, kc, vc, *a, **k):
            self.prefill_rows.append((x.shape[0], kc.shape[1], kc.shape[2]))
            return self.orig[2](x, kc, vc, *a, **k)
        self.eng.decode_step_shared, self.eng.decode_step, self.eng.prefill = shared, plain, prefill
        return self

    def __exit__(self, *a):
        del self.eng.decode_step_shared, self.eng.decode_step, self.eng.prefill


def planes(c):
    """A cache as the tensors to compare bit for bit: itself, or the code and exponent planes of an fp8 image."""
    return ops.kv8_unpack(c) if c.dtype == torch.uint8 else (c,)


# ---------------------------------------------------------------- step level
@pytest.mark.parametrize("case", ["bf16", "kv-fp8", "weights-fp4"])
def test_shared_step_against_the_copy_step(dev, tiny, m16, case):  # noqa: F811
    g, oc, W, audio, video, *_ = tiny
    m = {"bf16": lambda: m16, "kv-fp8": lambda: built(kv_cache="fp8"), "weights-fp4": lambda: built(decode_weights="fp4")}[case]()
    eng = m.llm_engine
    with torch.no_grad():
        x = m._llm_inputs(audio.to(dev), video.to(dev), None)
    B, S, _ = x.shape
    group, N = 3, 8
    R = B * group
    assert eng.decode_shares_prefix(R) and eng.decode_is_fused(R) and not eng.decode_shares_prefix(17)
    assert eng.decode_caches_fp8(R) == (case == "kv-fp8") and eng.decode_streams_fp4(R) == (case == "weights-fp4")
    kc0, vc0 = eng.alloc_cache(B, S, rows=R)
    eng.prefill(x, kc0, vc0)
    kc, vc = eng.alloc_cache(R, S + N)
    ks, vs = eng.alloc_suffix_cache(R, N)
    assert ks.dtype == kc0.dtype == kc.dtype == (torch.uint8 if case == "kv-fp8" else BF) and ks.shape[1:3] == (R, N)
    for t in (kc, vc, ks, vs):
        t.fill_(0xA5) if t.dtype == torch.uint8 else t.fill_(float("nan"))
    gather = ops.kv8_gather_rows if kc.dtype == torch.uint8 else ops.kv_gather_rows
    item = torch.arange(R, device=dev, dtype=torch.int32) // group
    gather(kc0, vc0, kc, vc, item, 0, S)
    gen = torch.Generator().manual_seed(11)
    ids = torch.randint(0, oc.llama.vocab, (R, N_NEW), generator=gen).to(dev)
    for cur in range(N_NEW):
        if cur:             # a reorder inside every item: a cycle, a parent taken twice
            perm = torch.tensor([[1, 2, 0], [0, 0, 2], [2, 1, 1]][cur % 3], dtype=torch.int32, device=dev)
            parent = (item * group + perm.repeat(B)).contiguous()
            gather(kc, vc, kc, vc, parent, S, S + cur)
            gather(ks, vs, ks, vs, parent, 0, cur)
        want = eng.decode_step(ids[:, cur].contiguous(), S + cur, kc, vc).clone()
        # the tiny model's shapes get the one-launch attention; odd steps force the two-launch form with two prefix slices
        with L.knob("SHARED_SPLIT", 2 * (cur % 2)):
            got = eng.decode_step_shared(ids[:, cur].contiguous(), cur, kc0, vc0, ks, vs, group)
        e = rel_l2(got, want)
        print(f"{case} step {cur}: shared vs copy logits relative L2 {e:.2e}")
        assert e < BF16_LOGITS_REL_L2
        # the writers are the same kernels at the same RoPE position: the suffix rows are the copy cache's generated rows
        for a, b in ((ks, kc), (vs, vc)):
            for pa, pb in zip(planes(a), planes(b)):
                diff = (pa[:, :, :cur + 1] != pb[:, :, S:S + cur + 1]).flatten(1).sum(1).tolist()
                print(f"{case} step {cur}: differing cache elements per layer {diff}")
                assert torch.equal(pa[:, :, :cur + 1], pb[:, :, S:S + cur + 1])
    # the position from device memory: the same step, bit for bit
    pd = torch.tensor([N_NEW - 1], device=dev, dtype=torch.int32)
    with L.knob("SHARED_SPLIT", 2 * ((N_NEW - 1) % 2)):
        assert torch.equal(eng.decode_step_shared(ids[:, N_NEW - 1].contiguous(), 0, kc0, vc0, ks, vs, group, pos_dev=pd), got)
    with pytest.raises(ValueError, match="group"):
        eng.decode_step_shared(ids[:, 0].contiguous(), 0, kc0, vc0, ks, vs, 2)


def test_memory_is_prefix_plus_suffix(dev, tiny, m16):  # noqa: F811
    g, oc, W, *_ = tiny
    lc = oc.llama
    dkv = (lc.kv_heads or lc.heads) * (lc.hidden // lc.heads)
    B, group, S, N = 2, 4, 37, 10
    R = B * group
    for eng, per in ((m16.llm_engine, 2.0), (built(kv_cache="fp8").llm_engine, 33 / 32)):
        pre, suf = eng.alloc_cache(B, S, rows=R), eng.alloc_suffix_cache(R, N)
        held = sum(t.numel() * t.element_size() for t in pre + suf)
        want = 2 * lc.layers * dkv * (B * S + R * N) * per                     # K and V, bytes per cached element
        assert held == eng.kv_cache_bytes(B, S) + eng.kv_cache_bytes(R, N) == want
        assert eng.kv_cache_bytes(R, S + N) == 2 * lc.layers * dkv * R * (S + N) * per > want


# ---------------------------------------------------------------- beam search
@pytest.mark.parametrize("nb", [2, 4])
def test_beam_scores_are_teacher_forced(dev, tiny, m16, nb):  # noqa: F811
    """test_generate_beam_gpu.py::test_bf16_fused_and_general_token_step's rule on B = 2 items; the per-token log-probabilities sum to the score."""
    g, oc, W, audio, video, *_ = tiny
    m, eos = m16, 239
    with with_eos(m, eos), Spy(m.llm_engine) as spy:
        out = m.generate(audio=audio.to(dev), video=video.to(dev), max_new_tokens=N_NEW, num_beams=nb, share_prefix=True, return_token_scores=True)
    B = audio.shape[0]
    assert spy.shared > 0 and spy.plain == 0 and [r[0] for r in spy.prefill_rows] == [B]
    ids, scores = out.sequences.cpu(), out.sequences_scores.cpu()
    with torch.no_grad():
        x = m._llm_inputs(audio.to(dev), video.to(dev), None)
    tot, lens = seq_logprob(m, x, ids, m.tokenizer.pad_token_id, eos, dev)
    print(f"share_prefix beams {nb}: scores {scores.tolist()}, teacher-forced {(tot / lens.double()).tolist()}")
    assert ((scores.double() - tot / lens.double()).abs() <= 4 * BF16_LOGIT_MAX_ABS).all(), (scores, tot / lens)
    assert ((out.token_scores.cpu().double().sum(1) / lens.double() - scores.double()).abs() <= 1e-4).all()


@pytest.mark.parametrize("nb", [2, 4])
def test_beam_scores_on_the_fp8_cache(dev, nb):
    """test_generate_kv8_gpu.py::test_beam_search_scores_are_the_references' rule, prefix and suffix both images."""
    oc, W, _, _ = K.tiny()
    sd, lora, c, lc = W["llama"], W["lora"], oc.llama, oc.lora
    audio, video, x = K.beam_inputs()
    m = built(kv_cache="fp8")
    assert m.llm_engine.decode_caches_fp8(K.BEAM_B * nb)
    with with_eos(m, K.BEAM_EOS), Spy(m.llm_engine) as spy:
        ids, scores = generate_ref.gen(m, audio, video, dev, K.BEAM_N, num_beams=nb, return_sequence_scores=True, share_prefix=True)
        greedy = generate_ref.gen(m, audio, video, dev, K.BEAM_N, share_prefix=True)
    assert spy.shared > 0 and spy.prefill_rows[0][0] == K.BEAM_B
    tot, lens, _ = R64.forced(sd, lora, c, lc, x, ids, K.BEAM_EOS)
    tol = 2.0 * BF16_LOGIT_MAX_ABS
    print(f"share_prefix beams {nb} kv_cache=fp8: scores {scores.tolist()}, reference along the same hypotheses {(tot / lens.double()).tolist()}")
    assert ((scores.double() - tot / lens.double()).abs() <= tol).all()
    gt, gl, _ = R64.forced(sd, lora, c, lc, x, greedy, K.BEAM_EOS)
    assert (scores.double() >= gt / gl.double() - tol).all()


# ---------------------------------------------------------------- sampled n-best
def test_sampled_nbest_prefills_once_per_item(dev, tiny, m16):  # noqa: F811
    g, oc, W, audio, video, *_ = tiny
    m, n = m16, 3
    B = audio.shape[0]
    kw = dict(audio=audio.to(dev), video=video.to(dev), max_new_tokens=N_NEW, do_sample=True, temperature=1.0, top_k=0, top_p=1.0, seed=5,
              num_return_sequences=n, return_token_scores=True)
    with with_eos(m, None), Spy(m.llm_engine) as spy:
        out = m.generate(share_prefix=True, **kw)
    with torch.no_grad():
        x = m._llm_inputs(audio.to(dev), video.to(dev), None)
    S = x.shape[1]
    assert spy.prefill_rows == [(B, B, S)] and spy.shared == N_NEW - 1 and spy.plain == 0      # B rows prefilled into a B-row cache of S positions
    with with_eos(m, None), Spy(m.llm_engine) as spy:
        plain = m.generate(**kw)
    assert spy.prefill_rows == [(B * n, B * n, S + N_NEW)] and spy.shared == 0
    ids = out.sequences
    assert ids.shape == (B * n, N_NEW) and torch.equal(ids[:, 0], plain.sequences[:, 0])         # step 0 draws from the same prefill logits
    assert len({tuple(r) for r in ids.tolist()}) > B, "the rows of an item draw with their own seeds"
    # teacher-forced: each row's own history after its item's prefix
    eng, xr = m.llm_engine, x.repeat_interleave(n, dim=0)
    worst = 0.0
    for j in range(N_NEW):
        xj = xr if j == 0 else torch.cat([xr, ops.embedding(eng.embed, ids[:, :j].contiguous())], 1)
        kc, vc = eng.alloc_cache(B * n, S + j)
        logits, _ = eng.prefill(xj.contiguous(), kc, vc)
        lp = torch.log_softmax(logits.float(), -1).gather(1, ids[:, j:j + 1])[:, 0]
        worst = max(worst, float((lp - out.token_scores[:, j]).abs().max()))
    print(f"sampled n-best on a shared prefix: worst |token log-probability - teacher-forced| {worst:.3e}")
    assert worst <= 2 * BF16_LOGIT_MAX_ABS


# ---------------------------------------------------------------- fallbacks and the default
def same(a, b):
    a, b = (tuple(t for t in o if t is not None) if isinstance(o, tuple) else (o,) for o in (a, b))
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def test_fallbacks_are_bit_equal(dev, tiny, m16):  # noqa: F811
    g, oc, W, audio, video, *_ = tiny
    a, v = audio.to(dev), video.to(dev)
    beam = dict(audio=a, video=v, max_new_tokens=4, return_token_scores=True)
    # 2 items x 16 beams = 32 rows: the general token step
    assert not m16.llm_engine.decode_shares_prefix(32)
    with Spy(m16.llm_engine) as spy:
        got = m16.generate(num_beams=16, share_prefix=True, **beam)
    assert spy.shared == 0 and same(got, m16.generate(num_beams=16, share_prefix=False, **beam))
    # fp32
    m32 = make_model(oc, W, "fp32", max_seq_len=256).eval()
    assert not m32.llm_engine.decode_shares_prefix(6)
    assert same(m32.generate(num_beams=3, share_prefix=True, **beam), m32.generate(num_beams=3, **beam))
    # greedy, and one sampled sequence per item: nothing to share
    with Spy(m16.llm_engine) as spy:
        assert same(m16.generate(share_prefix=True, **beam), m16.generate(**beam))
        samp = dict(do_sample=True, seed=3, **beam)
        assert same(m16.generate(share_prefix=True, **samp), m16.generate(**samp))
    assert spy.shared == 0
    # the fused step switched off
    with L.knob("DECODE_FUSED", 0):
        assert not m16.llm_engine.decode_shares_prefix(6)
        assert same(m16.generate(num_beams=3, share_prefix=True, **beam), m16.generate(num_beams=3, **beam))


def test_default_is_the_copy_path(dev, tiny, m16):  # noqa: F811
    """Without the keyword: share_prefix=False, no shared step, and the result of the fallback path of share_prefix=True bit for bit."""
    g, oc, W, audio, video, *_ = tiny
    kw = dict(audio=audio.to(dev), video=video.to(dev), max_new_tokens=N_NEW, num_beams=4, return_token_scores=True)
    with with_eos(m16, 239):
        with Spy(m16.llm_engine) as spy:
            default = m16.generate(**kw)
        assert spy.shared == 0 and spy.plain > 0
        assert same(default, m16.generate(share_prefix=False, **kw))
        with L.knob("DECODE_FUSED", 0):
            off = m16.generate(**kw)
            assert same(off, m16.generate(share_prefix=True, **kw))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="share_prefix"):
            m16.generate(share_prefix=bad, **kw)


def test_decode_py_share_prefix(dev, tmp_path):
    data, dec = tmp_path / "toy", tmp_path / "dec"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_toy_dataset.py"), str(data)], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts/clip_whisper/decode.py"), "--test_data", str(data / "test.tsv"),
                        "--test_wrd", str(data / "test.wrd"), "--output_dir", str(dec), "--modality", "both", "--batch_size", "2",
                        "--max_new_tokens", "4", "--tiny", "--data_path", str(data), "--share_prefix", "--num_beams", "4"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Overall WER:" in r.stdout
    assert open(glob.glob(str(dec / "wer_*.txt"))[0]).read().split("\n")[1] == "Total samples: 4"
    assert glob.glob(str(dec / "decode_results.json"))
