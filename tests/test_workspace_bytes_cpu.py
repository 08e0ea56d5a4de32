"""CPU: the workspace sizes the model entry points ask for (avllm_*_workspace_bytes: pure host code on descriptors, no device).

A caller allocates exactly these byte counts, so the order and the size of every buffer the entry points carve out of a workspace is part of
what callers observe, and no numerical test sees a slip in it until a buffer overlaps its neighbour.  The expected values are literals
recorded from the library as it stood before the encoder and Llama layouts were restated on shared helpers (csrc/engine.hip carve_enc and
the training frame): they were printed by that earlier build, not derived from the code under test."""
import ctypes as C

import pytest

from avllm import lib as L

PTR = 0x100000      # fake operand: non-null, never read


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    return L.load()


def whisper(d, heads, layers, ffn, n_mels=80, n_ctx=1500, dtype=L.BF16, fp8=0):
    w = L.Whisper()
    w.dtype, w.d, w.heads, w.layers, w.ffn, w.n_mels, w.n_ctx, w.k1pad = dtype, d, heads, layers, ffn, n_mels, n_ctx, (3 * n_mels + 63) // 64 * 64
    w.conv1_w = w.conv1_b = w.conv2_w = w.conv2_b = w.pos = w.lnf_w = w.lnf_b = PTR
    w.fp8 = fp8
    return w


def clip(d, heads, layers, ffn, image, patch, dtype=L.BF16, fp8=0):
    c = L.Clip()
    c.dtype, c.d, c.heads, c.layers, c.ffn, c.image, c.patch, c.tokens = dtype, d, heads, layers, ffn, image, patch, (image // patch) ** 2 + 1
    c.eps = 1e-5
    c.patch_w = c.class_emb = c.pos = c.pre_ln_w = c.pre_ln_b = PTR
    c.fp8 = fp8
    return c


def llama(d, heads, layers, ffn, vocab, kv_heads=0, dtype=L.BF16, fp8=0, r=16):
    m = L.Llama()
    m.dtype, m.d, m.heads, m.layers, m.ffn, m.vocab, m.lora_r, m.kv_heads = dtype, d, heads, layers, ffn, vocab, r, kv_heads
    m.eps, m.theta, m.lora_scale = 1e-5, 10000.0, 2.0
    m.embed = m.norm_w = m.lm_head = m.lm_head_t = PTR
    m.fp8 = fp8
    return m


# the tiny model of tests/test_lora_batch_gpu.py::test_batched_and_unbatched_steps_agree, and the BASELINE.md widths (Whisper-small, CLIP ViT-B/16,
# Llama-2-7B) with small B and S
WHISPER = {
    "tiny-bf16-B2": (whisper(128, 2, 2, 256), 2, 13056256),
    "tiny-fp32-B2": (whisper(128, 2, 2, 256, dtype=L.F32), 2, 26112256),
    "tiny-fp8-B2": (whisper(128, 2, 2, 256, fp8=1), 2, 13848832),
    "small-bf16-B1": (whisper(768, 12, 12, 3072), 1, 36096256),
    "small-fp8-B3": (whisper(768, 12, 12, 3072, fp8=1), 3, 122554624),
    "largev3-bf16-B1": (whisper(1280, 20, 32, 5120, n_mels=128), 1, 59904256),
}
CLIP = {
    "tiny-bf16-N14": (clip(128, 2, 2, 256, 48, 16), 14, 487680),
    "tiny-fp32-N14": (clip(128, 2, 2, 256, 48, 16, dtype=L.F32), 14, 975104),
    "tiny-fp8-N14": (clip(128, 2, 2, 256, 48, 16, fp8=1), 14, 525568),
    "b16-bf16-N3": (clip(768, 12, 12, 3072, 224, 16), 3, 9990400),
    "b16-fp8-N5": (clip(768, 12, 12, 3072, 224, 16, fp8=1), 5, 19774720),
    "l14-bf16-N2": (clip(1024, 16, 24, 4096, 224, 14), 2, 11190528),
}
#                                                       B, S, train, infer
LLAMA = {
    "tiny-bf16": (llama(256, 2, 2, 512, 256), 2, 64, 2922752, 983296),
    "tiny-fp32": (llama(256, 2, 2, 512, 256, dtype=L.F32), 2, 64, 5806336, 1786112),
    "tiny-fp8": (llama(256, 2, 2, 512, 256, fp8=1), 2, 64, 2992384, 983296),
    "tiny-kv1": (llama(256, 2, 2, 512, 256, kv_heads=1), 2, 64, 2726144, 917760),
    "tiny-odd-B3-S41": (llama(256, 2, 2, 512, 256), 3, 41, 2799104, 935168),
    "narrow-bf16": (llama(128, 1, 2, 256, 256), 2, 64, 1610496, 590080),
    "7b-bf16-L32": (llama(4096, 32, 32, 11008, 32000), 1, 8, 28014336, 1967360),
    "7b-fp8-L2": (llama(4096, 32, 2, 11008, 32000, fp8=1), 2, 16, 14487296, 7811328),
    "8b-gqa-bf16-L4": (llama(4096, 32, 4, 14336, 128256, kv_heads=8), 2, 16, 27327232, 20377856),
    "8b-gqa-fp32-L4": (llama(4096, 32, 4, 14336, 128256, kv_heads=8, dtype=L.F32), 1, 24, 40974080, 18245888),
}


@pytest.mark.parametrize("name", sorted(WHISPER))
def test_whisper_workspace_bytes(lib, name):
    w, B, want = WHISPER[name]
    assert lib.avllm_whisper_workspace_bytes(C.byref(w), B) == want


@pytest.mark.parametrize("name", sorted(CLIP))
def test_clip_workspace_bytes(lib, name):
    c, N, want = CLIP[name]
    assert lib.avllm_clip_workspace_bytes(C.byref(c), N) == want


@pytest.mark.parametrize("name", sorted(LLAMA))
def test_llama_workspace_bytes(lib, name):
    m, B, S, train, infer = LLAMA[name]
    assert lib.avllm_llama_train_workspace_bytes(C.byref(m), B, S) == train
    assert lib.avllm_llama_infer_workspace_bytes(C.byref(m), B, S) == infer


def test_train_workspace_of_a_model_past_the_layer_limit_is_zero(lib):
    assert lib.avllm_llama_train_workspace_bytes(C.byref(llama(256, 2, 257, 512, 256)), 2, 64) == 0
    assert lib.avllm_llama_train_workspace_bytes(None, 2, 64) == 0
