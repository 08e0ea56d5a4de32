"""The decode-time LoRA merge on the CPU, before the GPU tests lean on it: merging in float64 is the same function as the adapters; the bar of
tests/bars_merge.py holds a faithful fp32 restatement of the kernel's arithmetic and not a wrong one; and the inputs of
tests/test_generate_merged_gpu.py (tests/refs64_merge.py) are such that its comparisons say something: without the adapters the logits are
far outside the bf16 bar, with them merged on the host and rounded to bf16 they are well inside it, and the reference's decisions are clear, and
held by the host-merged model, often enough."""
import torch

import kv8_cases as K
import refs64_kv8 as R
import refs64_merge as M
from avllm import lib as L
from bars import BF16_LOGITS_REL_L2, rel_l2
from bars_merge import merge_bar


def test_abi_name_is_exported():
    assert "avllm_lora_merge" in L.EXPORTS
    assert L.Llama._fields_[-1][0] == "kv_fp8", "the merge adds no field to avllm_llama"


def test_merged_float64_weights_are_the_adapters():
    oc, W = M.tiny()
    _, _, x = K.greedy_inputs()
    sd, lora = W["llama"], W["lora"]
    merged = M.merged_sd64(sd, lora, oc.llama.layers, oc.lora.scale)
    with_adapters = M.prefill_logits64(sd, lora, oc, x)
    e = rel_l2(M.prefill_logits64(merged, None, oc, x), with_adapters)
    print(f"float64 merge vs adapters, prefill logits: relative L2 {e:.2e}")
    assert e < 1e-5                      # the bar of test_kv8_refs_cpu's fp32 comparison; float64 reassociation of (x A^T) B^T is far below it


def _kernel_restated_fp32(W, A, B, scale, dtype):
    """The header's arithmetic on the host in fp32: ascending chain (each step a rounded product and a rounded sum, which the fused chain of the
    kernel is at least as exact as), a rounded product with scale, a rounded sum, one rounding to the storage type."""
    u = torch.zeros(W.shape, dtype=torch.float32)
    for j in range(A.shape[0]):
        u = u + B[:, j:j + 1] * A[j:j + 1, :]
    return (W.float() + torch.tensor(scale, dtype=torch.float32) * u).to(dtype)


def test_bar_holds_a_faithful_restatement_and_not_a_wrong_one():
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.float32, torch.bfloat16):
        for r, scale in ((1, 2.0), (16, -0.5), (64, 2.0)):
            A, B = torch.randn(r, 264, generator=g), torch.randn(130, r, generator=g)
            for family in ("gauss", "offset"):
                W = torch.randn(130, 264, generator=g)
                if family == "offset":
                    W = (-scale * (B.double() @ A.double()) + 1e-3 * W.double()).float()
                W = W.to(dtype)
                ref, u, sum_abs = M.merge64(W, A, B, scale)
                bar = merge_bar(ref, u, sum_abs, r, scale, dtype == torch.bfloat16)
                err = (_kernel_restated_fp32(W, A, B, scale, dtype).double() - ref).abs()
                print(f"{family} {dtype} r={r}: worst error / bar {float((err / bar).max()):.3f}")
                assert bool((err <= bar).all())
                # a dropped rank step is outside it; so are, for an f32 store (a bf16 store's own rounding is as large), the adapter path's
                # bf16 operands in place of the fp32 masters
                if r > 1:
                    wrong = _kernel_restated_fp32(W, A[:-1], B[:, :-1], scale, dtype).double()
                    assert not bool(((wrong - ref).abs() <= bar).all())
                if dtype == torch.float32:
                    wrong = _kernel_restated_fp32(W, A.to(torch.bfloat16).float(), B.to(torch.bfloat16).float(), scale, dtype).double()
                    assert not bool(((wrong - ref).abs() <= bar).all())


def test_premises_of_the_generate_tests():
    oc, W = M.tiny()
    _, _, x = K.greedy_inputs()
    sd, lora, c, lc = W["llama"], W["lora"], oc.llama, oc.lora
    host_merged = M.bf16_round(M.merged_sd64(sd, lora, c.layers, lc.scale))
    want = M.prefill_logits64(sd, lora, oc, x)
    dropped = rel_l2(M.prefill_logits64(sd, None, oc, x), want)
    merged = rel_l2(M.prefill_logits64(host_merged, None, oc, x), want)
    print(f"prefill logits against the adapter reference: no adapters {dropped:.2e}, host-merged bf16 weights {merged:.2e}")
    assert dropped >= 3 * BF16_LOGITS_REL_L2, "a merge that silently drops the term must not pass the GPU test"
    assert merged < BF16_LOGITS_REL_L2
    eos, pad = 2, oc.pad_token_id
    ref, margins = R.greedy(sd, lora, c, lc, x, K.N_GREEDY, eos, pad, store=R.identity)
    clear = R.held_decisions(ref, ref, margins, K.threshold())
    ids, _ = R.greedy(host_merged, None, c, None, x, K.N_GREEDY, eos, pad, store=R.identity)
    held = R.held_decisions(ids, ref, margins, K.threshold())
    print(f"greedy: {clear} of {margins.numel()} reference decisions are clear at {K.threshold()}; the host-merged model holds {held}")
    assert clear >= K.MIN_HELD and held >= K.MIN_HELD
