"""The training step of LlamaEngine (csrc/engine.hip avllm_llama_lora_fwd_loss, avllm_llama_lora_bwd_layers_dx) on every case of
tests/train_step_cases.py: head geometry x precision x adapted modules x rank x dropout (off, seed in the descriptor, seed split with a device
word) x head norms x biases x RoPE rule x rows x the pieces of the backward, against the float64 step of tests/refs64_lora_mlp.py.
tests/test_train_step_cases_cpu.py shows on the host that the case list holds every pair of levels, that the reference is transformers'
arithmetic (and the oracle's in fp8 form), that a correct bf16 forward has half the logits bar to itself in every case and that a step with one
feature wrong misses the bars.

Per case: one fwd_loss(want_logits=True) and the backward in the case's pieces, with the after_layer callback recorded; under dropout the
reference is fed the masks the kernels generate (avllm_dropout at every module's input width with the module's seed: the materialising
kernel, the in-GEMM generators of the forward, of dA and of the input gradient have to agree with it).  Loss, logits, every adapter gradient
and (unless the case passes no buffer) dx_embeds are held to the bars of tests/bars.py for the case's precision through
train_step_cases.ratios, which applies them as tests/test_lora_mlp_gpu.py does; fp8 cases against the reference with the frozen products
fake-quantised.  The worst error / bar of every quantity is printed per case (RATIO lines).

Measured on MI355X, worst error / bar over the cases of a precision ("The training step across pairings", has every case):
  bf16 (9 cases): loss 0.002 .. 0.131, logits 0.358 .. 0.477, whole gradient 0.196 .. 0.317, worst tensor 0.135 .. 0.229, dx_embeds 0.103 .. 0.170;
  fp8 (5 cases):  loss 0.011 .. 0.198, logits 0.534 .. 0.690, whole gradient 0.326 .. 0.455, dx_embeds 0.317 .. 0.437 (worst tensor over the
                  whole-gradient bar, printed only: 0.583 .. 0.723);
  fp32 (7 cases): loss <= 0.012, logits <= 0.017, worst tensor <= 0.022, dx_embeds <= 0.013.
The bf16 gradient figures are the gradients' headroom, which has no rounded restatement on the host: a correct engine uses a third of the bar.
Controls: masks of another base seed miss the gradient bar 19 .. 25 x (bf16), 5.5 .. 6.5 x (fp8), 5800 .. 8300 x (fp32); the descriptor's seed
without the device word the same.  22 tests, 5 s."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import refs64_lora_mlp as R  # noqa: E402
import train_step_cases as TC  # noqa: E402

F32 = torch.float32


def build(dev, c):
    from avllm.engine import LlamaEngine
    sd, lora = TC.weights(c)
    return LlamaEngine(sd, TC.llama_cfg(c), TC.lora_cfg(c), lora, dtype=TC.engine_dtype(c), device=dev, training=True, fp8=c.precision == "fp8")


def device_word(dev, value):
    """A uint32 in device memory (held as the int32 of the same bits)."""
    return torch.tensor([value - (1 << 32) if value >= (1 << 31) else value], dtype=torch.int32, device=dev)


def forward(dev, eng, c, x, labels, word):
    _, host, _ = TC.seeds(c)
    return eng.fwd_loss(x, labels, want_logits=True, dropout=c.p, seed=host if c.p else 0, seed_dev=word.data_ptr() if word is not None else None)


def backward(dev, eng, c, pieces, **kw):
    """The backward in `pieces` -> (dx_embeds on the device or None, the layers the callback saw, in order)."""
    order = []
    dx = None if pieces == "nodx" else torch.full((c.B, c.S, c.hidden), float("nan"), device=dev, dtype=eng.dtype)
    eng.lora_g.zero_()
    if pieces == "split":
        eng.bwd(after_layer=order.append, layer_hi=1, layer_lo=1, **kw)
        eng.bwd(after_layer=order.append, layer_hi=0, layer_lo=0, dx_embeds=dx, **kw)
    elif pieces == "whole":
        eng.bwd(after_layer=order.append, dx_embeds=dx, **kw)
    else:
        eng.bwd(after_layer=order.append, **kw)
    torch.cuda.synchronize()
    return dx, order


def kernel_masks(dev, c, base):
    """The step's masks as the kernels generate them for base seed `base`: ops.dropout(ones [M, K], seed_of(base, l, module), p)."""
    from avllm import ops
    out = {}
    for l in range(c.layers):
        for nm in c.modules:
            K = c.ffn if nm == "down_proj" else c.hidden
            m = ops.dropout(torch.ones(c.B * c.S, K, device=dev, dtype=F32), R.seed_of(base, c.layers, l, nm), c.p)
            out[f"layers.{l}.{nm}"] = m.cpu().view(c.B, c.S, K).double()
    return out


def grad_ratio(r):
    """The gradient ratio of train_step_cases.ratios the mask controls look at: the whole gradient (bf16, fp8), the worst tensor (fp32)."""
    return r["grad"] if "grad" in r else r["tensor"]


def collect(eng, loss_of, logits, dx):
    grads = {k: v.detach().cpu().clone() for k, v in eng.lora_views(eng.lora_g).items()}
    return loss_of, logits.float().cpu(), grads, None if dx is None else dx.float().cpu()


@pytest.mark.parametrize("c", TC.CASES, ids=lambda c: c.id)
def test_train_step_matrix(dev, c):
    eng = build(dev, c)
    assert eng.targets == tuple(c.modules) and eng.fp8 == (c.precision == "fp8")
    x, labels = TC.inputs(c)
    xg, lg = x.to(dev, eng.dtype), labels.to(dev)
    base, host, devw = TC.seeds(c)
    word = device_word(dev, devw) if devw is not None else None

    logits = forward(dev, eng, c, xg, lg, word)
    loss = float(eng.acc[0] / eng.acc[1])
    assert int(eng.acc[1]) == int((labels[:, 1:] != -100).sum())
    dx, order = backward(dev, eng, c, c.pieces)
    assert order == [1, 0], order
    got = collect(eng, loss, logits, dx)
    assert all(bool(torch.isfinite(t).all()) for t in (got[1], *got[2].values())) and (dx is None or bool(torch.isfinite(got[3]).all()))

    masks = kernel_masks(dev, c, base) if c.p else None
    if masks is not None:
        assert len({int((m != 0).sum()) for m in masks.values()}) > 1, "one mask for every module"
        assert all(abs(float((m != 0).double().mean()) - (1 - c.p)) < 0.02 for m in masks.values())
    ref = TC.ref_step(c, masks)
    if dx is None:
        ref = ref[:3] + (None,)
    r = TC.ratios(c, got, ref)
    print(f"RATIO {c.id}: {TC.show(r)}")
    assert TC.worst(r) < 1.0, r

    # ---- controls
    if c.p:      # the masks are really applied, and the same ones in the forward, in dA and in the input gradient: another base seed's are far off
        other = TC.ratios(c, got, TC.ref_step(c, kernel_masks(dev, c, (base + 1000) & 0xFFFFFFFF))[:3] + (ref[3],))
        print(f"CONTROL {c.id}: masks of base + 1000: gradient error / bar {grad_ratio(other):.1f}")
        assert grad_ratio(other) > 4.0
    if devw is not None:      # and the device word is part of the seed
        alone = TC.ratios(c, got, TC.ref_step(c, kernel_masks(dev, c, host))[:3] + (ref[3],))
        print(f"CONTROL {c.id}: masks of the descriptor's seed without the device word: gradient error / bar {grad_ratio(alone):.1f}")
        assert grad_ratio(alone) > 4.0
    again = forward(dev, eng, c, xg, lg, word)
    assert torch.equal(again, logits), "a second forward with the same seed is another forward"


def test_data_parallel_scaling(dev):
    """bwd(grad_scale=0.5, count=2 x the own count): every gradient is the reference's x 0.25, within the same bars, in both pieces."""
    c = TC.BY_NAME["default-deployment"]
    eng = build(dev, c)
    x, labels = TC.inputs(c)
    base, _, devw = TC.seeds(c)
    word = device_word(dev, devw)
    logits = forward(dev, eng, c, x.to(dev, eng.dtype), labels.to(dev), word)
    loss = float(eng.acc[0] / eng.acc[1])
    count = (2.0 * eng.acc[1:2]).clone()
    dx, order = backward(dev, eng, c, c.pieces, grad_scale=0.5, count=count)
    assert order == [1, 0]
    rl, rlogits, rg, rdx = TC.ref_step(c, kernel_masks(dev, c, base))
    r = TC.ratios(c, collect(eng, loss, logits, dx), (rl, rlogits, {k: 0.25 * v for k, v in rg.items()}, 0.25 * rdx))
    print(f"RATIO {c.id} grad_scale 0.5, count x 2: {TC.show(r)}")
    assert TC.worst(r) < 1.0, r
