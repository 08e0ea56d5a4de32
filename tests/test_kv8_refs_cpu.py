"""tests/refs64_kv8.py checked on the CPU before the GPU tests lean on it: with storage switched to identity it is the oracle's llama_hidden with
a cache; its quantiser is oracle/mxfp8.py's; what it stores is exactly representable in bf16 (so the kernels' in-register dequantisation can be
exact); and on the inputs the GPU tests use (tests/kv8_cases.py) its own decisions are clear (top-2 margin >= 2 x BF16_LOGIT_MAX_ABS) at least
MIN_HELD times, so following it at that threshold is not vacuous."""
import torch

import kv8_cases as K
import refs64_kv8 as R
from avllm import lib as L
from bars import rel_l2
from oracle import avsr_oracle as O
from oracle import mxfp8


def test_identity_storage_is_llama_hidden_with_past():
    oc, W, _, _ = K.tiny()
    sd, lora, c, lc = W["llama"], W["lora"], oc.llama, oc.lora
    _, _, x = K.greedy_inputs()
    x = x[:2]
    S = x.shape[1]
    g = torch.Generator().manual_seed(0)
    toks = torch.randint(0, c.vocab, (2, 3), generator=g)
    po, pr = [None] * c.layers, [None] * c.layers
    with torch.no_grad():
        for t in range(4):
            xi = x if t == 0 else sd["model.embed_tokens.weight"][toks[:, t - 1]][:, None]
            pos0 = 0 if t == 0 else S + t - 1
            ho = O.llama_hidden(sd, lora, c, lc, xi, past=po, pos0=pos0)
            hr = R.llama_hidden(sd, lora, c, lc, xi, pr, pos0, store=R.identity)
            e = rel_l2(ho, hr)
            print(f"step {t}: llama_hidden (fp32) vs refs64_kv8 with identity storage, relative L2 {e:.2e}")
            assert e < 1e-5                                      # fp32 round-off of a 2-layer model: ~1e-7 per operation, a few hundred in a chain
    # and storage changes the steps, not the prefill
    pq = [None] * c.layers
    with torch.no_grad():
        h0 = R.llama_hidden(sd, lora, c, lc, x, pq, 0)
        assert torch.equal(h0, R.llama_hidden(sd, lora, c, lc, x, [None] * c.layers, 0, store=R.identity))
        xi = sd["model.embed_tokens.weight"][toks[:, 0]][:, None]
        h1 = R.llama_hidden(sd, lora, c, lc, xi, pq, S)
        h1i = R.llama_hidden(sd, lora, c, lc, xi, pr[:0] + [(k[:, :, :S], v[:, :, :S]) for k, v in pr], S, store=R.identity)
    d = rel_l2(h1, h1i)
    print(f"stored vs unstored cache, first step: relative L2 {d:.2e}")
    assert 1e-4 < d < 0.2


def test_quantiser_is_the_oracles_and_stores_bf16_values():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(64, 256, generator=g) * torch.logspace(-6, 6, 64, base=2.0)[:, None]
    x[0, :32] = 0.0                                              # amax == 0: exponent -127
    x[1, :32] = x[1, :32].clamp(-0.9, 0.9); x[1, 5] = 1.9375      # saturates: 496 / 256 of its power of two
    x[2, :32] = torch.arange(32) * 2.0 ** -4 * 17                 # exact ties of the e4m3 grid among them
    x[3, :32] = 2.0 ** -140                                       # subnormal amax
    x = x.to(torch.bfloat16).float()
    cq, ce = mxfp8.quantize(x)
    rq, re = R.mx_quantize64(x.double())
    assert torch.equal(re, ce) and torch.equal(rq, cq)
    assert int(ce[0, 0]) == -127 and bool((cq[1, :32].view(torch.float8_e4m3fn).float().abs() == 448).any())
    assert torch.equal(R.mx_dequantize64(rq, re).float(), mxfp8.dequantize(cq, ce))
    y = torch.randn(16, 128, generator=g, dtype=torch.float64) * 3.0          # float64 inputs, as the reference stores them
    s = R.mx_store(y)
    assert torch.equal(s.to(torch.bfloat16).double(), s), "code x 2^e has 4 significant bits: a bf16 value"
    assert torch.equal(R.mx_store(s), s), "storing is idempotent"
    # relative to the block's maximum: half a step of the top binade (16 / 256) at most, or the saturation of a maximum above 448 / 512 of its
    # power of two (64 / 512)
    assert float(((s - y).abs() / y.abs().view(16, 4, 32).amax(-1, keepdim=True).expand(16, 4, 32).reshape(16, 128)).max()) <= 2.0 ** -3


def test_abi_names_are_exported():
    for name in ("avllm_kv8_append", "avllm_kv8_rope_append", "avllm_attention_decode_kv8", "avllm_kv8_gather_rows", "avllm_llama_decode_caches_fp8",
                 "avllm_llama_kv_cache_bytes"):
        assert name in L.EXPORTS
    assert L.Llama._fields_[-1][0] == "kv_fp8"


def test_greedy_reference_decisions_are_clear_often_enough():
    thr = K.threshold()
    for with_lora in (False, True):
        oc, W, _, _ = K.tiny(with_lora)
        _, _, x = K.greedy_inputs()
        ids, margins = R.greedy(W["llama"], W.get("lora"), oc.llama, oc.lora, x, K.N_GREEDY, 2, oc.pad_token_id)
        held = R.held_decisions(ids, ids, margins, thr)
        print(f"tiny model, adapters {with_lora}: {held} of {margins.numel()} decisions have a margin >= {thr}")
        assert held >= K.MIN_HELD


def test_qwen3_reference_decisions_are_clear_often_enough():
    c, sd, lora, x = K.qwen3_inputs()
    from types import SimpleNamespace
    ids, margins = R.greedy(sd, lora, c, SimpleNamespace(scale=2.0), x, K.QWEN3_NEW, None, 0)
    held = R.held_decisions(ids, ids, margins, K.threshold())
    print(f"Qwen3 case a: {held} of {margins.numel()} decisions have a margin >= {K.threshold()}")
    assert held >= K.MIN_HELD


def test_beam_reference_steps_are_clear_often_enough():
    """Beam search is held to the reference through teacher-forced scores (test_generate_kv8_gpu.py); along the reference's own best hypotheses
    at least MIN_HELD steps have a clear top-2 margin, so those scores are sums over peaked distributions, not over near-ties only."""
    import generate_ref
    oc, W, _, _ = K.tiny()
    _, _, x = K.beam_inputs()
    sd, lora, c, lc = W["llama"], W["lora"], oc.llama, oc.lora
    seq, sc, gap = generate_ref.hf_beam_search(R.step_fn(sd, lora, c, lc, x, K.BEAM_NB), K.BEAM_B, K.BEAM_NB, c.vocab, K.BEAM_N, K.BEAM_EOS, oc.pad_token_id)
    tot, lens, margins = R.forced(sd, lora, c, lc, x, seq, K.BEAM_EOS)
    print(f"beam reference: lengths {lens.tolist()}, scores {sc.tolist()}, smallest selection gap {gap:.4f}, margins {[round(m, 3) for m in margins]}")
    assert ((tot / lens.double()).float() - sc).abs().max() < 1e-4, "hf_beam_search's scores are the teacher-forced mean log-probabilities"
    assert sum(m >= K.threshold() for m in margins) >= K.MIN_HELD
