"""The library calls of ClipWhisperModel.generate() after the encoders, per decoding mode, on the tiny fp32 model with 3 new tokens and no
EOS: which decoding entry of libavllm.so is called, in which order.  generate() promises that a keyword at its default launches nothing:
a processor, a score or a sampling call appears in a mode's sequence only where its keyword asks for it.  The calls are recorded by a
proxy in place of the loaded library (avllm.lib._lib) from the moment _llm_inputs returns; the two names of one kernel count as one."""
import pytest

pytestmark = pytest.mark.gpu

from avllm import lib as L  # noqa: E402
from generate_ref import with_eos  # noqa: E402
from test_model_gpu import make_model, tiny  # noqa: E402,F401

N = 3
P, D, A, S, R, LP, BT, KV = "llama_prefill", "llama_decode_step", "argmax_rows", "sample_rows", "row_scores", "logits_process", "beam_topk", \
    "kv_gather_rows"
# the decoding family: library entry -> the name it is recorded under
FAMILY = {"avllm_llama_prefill": P, "avllm_llama_decode_step": D, "avllm_llama_decode_step_at": D, "avllm_argmax_rows": A,
          "avllm_sample_rows": S, "avllm_sample_rows_scored": S, "avllm_row_scores": R, "avllm_row_scores_logprobs": R,
          "avllm_logits_process": LP, "avllm_logits_process_ex": LP, "avllm_beam_topk": BT, "avllm_beam_topk_logprobs": BT,
          "avllm_kv_gather_rows": KV}
SAMPLE = dict(do_sample=True, seed=1)
CASES = {
    "greedy": ({}, [P, A, D, A, D, A]),
    "greedy_ngram": (dict(no_repeat_ngram_size=2), [P, LP, A, D, LP, A, D, LP, A]),
    "greedy_suppress": (dict(suppress_tokens=[3]), [P, LP, A, D, LP, A, D, LP, A]),
    "greedy_scores": (dict(return_token_scores=True), [P, A, R, D, A, R, D, A, R]),
    "sampled": (SAMPLE, [P, S, D, S, D, S]),
    "sampled_scores": (dict(SAMPLE, return_token_scores=True), [P, S, R, D, S, R, D, S, R]),
    "beams": (dict(num_beams=2), [P, KV, BT, KV, D, BT, KV, D, BT]),
    "beams_ngram": (dict(num_beams=2, no_repeat_ngram_size=2), [P, KV, LP, BT, KV, D, LP, BT, KV, D, LP, BT]),
    "beams_suppress": (dict(num_beams=2, suppress_tokens=[3]), [P, KV, LP, BT, KV, D, LP, BT, KV, D, LP, BT]),
    "beams_scores": (dict(num_beams=2, return_token_scores=True), [P, KV, BT, R, KV, D, BT, R, KV, D, BT, R]),
}


class Recorder:
    """Forwards every attribute to the loaded library; a call of a FAMILY entry is noted first, while `on`."""

    def __init__(self, lib):
        self._lib, self.calls, self.on = lib, [], False

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in FAMILY:
            return fn

        def call(*args):
            if self.on:
                self.calls.append(FAMILY[name])
            return fn(*args)
        return call


@pytest.fixture(scope="module")
def m32(dev, tiny):  # noqa: F811
    g, oc, W, *_ = tiny
    return make_model(oc, W, "fp32", max_seq_len=256).eval()


@pytest.mark.parametrize("case", list(CASES))
def test_library_calls_of_each_mode(dev, tiny, m32, monkeypatch, case):  # noqa: F811
    g, oc, W, audio, video, labels, prompt = tiny
    kw, want = CASES[case]
    rec = Recorder(L.load())
    llm_inputs = m32._llm_inputs

    def recorded_from_here(*a, **k):
        x = llm_inputs(*a, **k)
        rec.on = True
        return x
    monkeypatch.setattr(L, "_lib", rec)
    monkeypatch.setattr(m32, "_llm_inputs", recorded_from_here)
    with with_eos(m32, None):
        out = m32.generate(audio=audio.to(dev), video=video.to(dev), max_new_tokens=N, **kw)
    ids = out[0] if isinstance(out, tuple) else out
    assert ids.shape == (audio.shape[0], N)
    assert rec.calls == want, (case, rec.calls)
