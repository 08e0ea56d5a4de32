"""The NumPy restatement of the sampling chain of ops.sample_rows (csrc/sample.hip), shared by the sampling tests and their references: HF's
TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper (min_tokens_to_keep = 1) with this build's tie rule: in descending order the
kept set is the shortest prefix whose tail mass is <= 1 - top_p, plus every token whose scaled logit equals that of the last kept one.
tests/test_sample_gpu.py holds it to HF's own classes.  A leaf module: it imports nothing of the test-suite and nothing of avllm."""
import numpy as np
import torch


def kept_from_scaled(x, top_k, top_p):
    """Boolean mask of the kept tokens and their probabilities, x = scaled logits (float64)."""
    V = x.shape[0]
    if top_k == 1:
        keep = np.zeros(V, bool)
        keep[int(np.argmax(x))] = True
        return keep, keep.astype(np.float64)
    keep = x > -np.inf
    if 0 < top_k < V:
        kth = np.sort(x)[::-1][top_k - 1]
        keep &= x >= kth
    m = x[keep].max()
    if top_p < 1.0:
        xs = x[keep]
        w = np.exp(xs - m)
        order = np.argsort(-xs, kind="stable")
        S = np.cumsum(w[order])
        j = int(np.argmax(S >= top_p * S[-1]))
        keep &= x >= xs[order][j]
    w = np.where(keep, np.exp(np.where(keep, x, m) - m), 0.0)
    return keep, w / w.sum()


def kept(row, temperature, top_k, top_p):
    """row: one row of logits as the kernel sees it (fp32 values; bf16 rows upcast exactly); the division happens in fp32 as on the device."""
    r = np.asarray(row, np.float32)
    t = np.float32(1.0 if top_k == 1 else temperature)
    return kept_from_scaled((r / t).astype(np.float64), top_k, top_p)


def rows(B, V, seed, scale=3.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * scale).to(dtype)
