"""ClipWhisperModel.generate(do_sample=True) on the tiny golden model (tests/golden/g2_tiny_e2e.npz): the sampled token step (ops.sample_rows)
inside the prefill / decode-step loop, and scripts/clip_whisper/decode.py --do_sample.  The kept-set restatement is test_sample_gpu.kept."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from avllm import ops  # noqa: E402
from test_model_gpu import T, make_model, tiny  # noqa: E402,F401
from test_sample_gpu import kept  # noqa: E402

# teacher-forced logits vs the decode step's: at positions whose kept-set boundary margin (scaled logits) is at least BOUNDARY_TOL the token
# must be in the kept set; at the others (bf16: the prefill and decode-step paths round differently, and the tiny model's 256 logits lie
# close together) its scaled logit must lie within 2 * BOUNDARY_TOL of the lowest kept one
BOUNDARY_TOL = {"fp32": 1e-3, "bf16": 6e-2}


def gen(m, audio, video, dev, **kw):
    return m.generate(audio=audio.to(dev), video=video.to(dev), max_new_tokens=12, **kw).cpu()


@pytest.fixture(scope="module")
def m32(dev, tiny):  # noqa: F811
    g, oc, W, *_ = tiny
    return make_model(oc, W, "fp32", max_seq_len=256).eval()


def test_top_k_1_equals_greedy_golden(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    ids = gen(m32, audio, video, dev, do_sample=True, top_k=1, top_p=0.9, temperature=0.7, seed=5)
    assert torch.equal(ids, T(g["generate_ids"])), (ids, g["generate_ids"])


def test_greedy_ignores_sampling_arguments(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    ids = gen(m32, audio, video, dev, do_sample=False, temperature=0.3, top_k=3, top_p=0.2)
    assert torch.equal(ids, T(g["generate_ids"]))


def test_manual_seed_repeats(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    torch.manual_seed(123)
    a = gen(m32, audio, video, dev, do_sample=True)
    torch.manual_seed(123)
    b = gen(m32, audio, video, dev, do_sample=True)
    assert torch.equal(a, b)
    c = gen(m32, audio, video, dev, do_sample=True, temperature=1.5, top_k=0, top_p=0.99, seed=1)
    d = gen(m32, audio, video, dev, do_sample=True, temperature=1.5, top_k=0, top_p=0.99, seed=2)
    assert not torch.equal(c, d)


def test_bad_arguments(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    for kw in ({"temperature": 0.0}, {"temperature": -1.0}, {"top_p": 0.0}, {"top_p": 1.2}, {"top_k": -1}):
        with pytest.raises(ValueError):
            gen(m32, audio, video, dev, do_sample=True, **kw)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("t,k,p", [(1.0, 50, 0.9), (0.7, 0, 0.8), (1.3, 20, 1.0)])
def test_teacher_forced_membership(dev, tiny, precision, t, k, p):  # noqa: F811
    """Each sampled token lies in the kept set of the logits an eval forward gives for the prompt plus the tokens before it."""
    g, oc, W, audio, video, labels, prompt = tiny
    m = make_model(oc, W, precision, max_seq_len=256).eval()
    m.eos_token_id = None                                   # every position is a real draw
    ids = gen(m, audio, video, dev, do_sample=True, temperature=t, top_k=k, top_p=p, seed=11)
    eng = m.llm_engine
    with torch.no_grad():
        x = m._llm_inputs(audio.to(dev), video.to(dev), None)
    B, S, _ = x.shape
    checked = 0
    for j in range(ids.shape[1]):
        xj = torch.cat([x, ops.embedding(eng.embed, ids[:, :j].to(dev).contiguous())], 1) if j else x
        kc, vc = eng.alloc_cache(B, S + j)
        logits, _ = eng.prefill(xj, kc, vc)
        lf = logits.float().cpu().numpy()
        for b in range(B):
            keep, _ = kept(lf[b], t, k, p)
            xs = lf[b] / np.float32(t)
            margin = xs[keep].min() - (xs[~keep].max() if (~keep).any() else -np.inf)
            tok = int(ids[b, j])
            if margin >= BOUNDARY_TOL[precision]:
                assert keep[tok], (precision, j, b, tok)
                checked += 1
            else:
                assert xs[tok] >= xs[keep].min() - 2 * BOUNDARY_TOL[precision], (precision, j, b, tok, xs[tok], xs[keep].min())
    assert precision != "fp32" or checked >= ids.numel() // 2, checked


def test_rows_that_emit_eos_are_padded(dev, tiny, m32):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    eos0 = m32.eos_token_id
    try:
        m32.eos_token_id = None
        free = gen(m32, audio, video, dev, do_sample=True, top_k=0, top_p=0.95, seed=21)
        eos = int(free[0, 2])
        m32.eos_token_id = eos
        got = gen(m32, audio, video, dev, do_sample=True, top_k=0, top_p=0.95, seed=21)
    finally:
        m32.eos_token_id = eos0
    pad = m32.tokenizer.pad_token_id
    want = free.clone()
    for b in range(want.shape[0]):
        hit = (free[b] == eos).nonzero()
        if len(hit):
            want[b, int(hit[0]) + 1:] = pad
    assert torch.equal(got, want[:, :got.shape[1]]), (got, want)
    assert (got[0, 3:] == pad).all()


def test_decode_script_sampling(dev, tmp_path):
    """decode.py --do_sample --top_p 0.9 --seed 1 twice: identical results; without --do_sample the output is greedy whatever --temperature
    says, and equals --do_sample --top_k 1."""
    from test_data_cpu import make_set
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = tmp_path / "toy"
    data.mkdir()
    mp, lp = make_set(data, n=4)
    env = dict(os.environ, PYTHONPATH=root)

    def run(name, *extra):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(root, "scripts/clip_whisper/decode.py"), "--test_data", str(mp), "--test_wrd", str(lp),
                            "--output_dir", str(out), "--batch_size", "2", "--max_new_tokens", "6", "--tiny", "--data_path", str(data), *extra],
                           capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return [x["hypothesis"] for x in json.load(open(glob.glob(str(out / "decode_results.json"))[0]))["results"]]

    s1 = run("s1", "--do_sample", "--top_p", "0.9", "--seed", "1")
    s2 = run("s2", "--do_sample", "--top_p", "0.9", "--seed", "1")
    assert s1 == s2 and len(s1) == 4
    greedy = run("g", "--temperature", "0.3", "--top_p", "0.5", "--top_k", "3")
    assert greedy == run("k1", "--do_sample", "--top_k", "1", "--seed", "9")
