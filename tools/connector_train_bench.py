#!/usr/bin/env python3
"""Times the launches train_connectors=True adds to a step at the bench shape (B = 16, S = 256, Llama-2-7B widths, whisper-small / ViT-B/16
widths, 125 frames; bf16, LoRA dropout 0.05 as bench.py runs): layer 0's dqkv . Wqkv product, the three adapters' masked input gradient and
the input-RMSNorm backward, the fusion / pooling adjoint, the two weight gradients with their bias sums, the refresh of the two bf16 operand
images; and the optimizer's two launches in both forms (flag on: one norm and one AdamW over connector + LoRA buffers; flag off: the LoRA
buffer alone), of which only the DIFFERENCE is added by the flag.  Prints per-launch times (device events) and their sum against the derived 0.45 ms; run it under
`rocprofv3 --kernel-trace --stats -- python tools/connector_train_bench.py` (a process of its own, no counters) for the kernels' own durations.
Next to it, as a yardstick only (torch is never on the product path): avllm_gemm_wgrad against torch's dY.t() @ X in bf16, alternating."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import lib as L
from avllm import ops


def timed(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1000


dev, bf = "cuda", torch.bfloat16
B, S, d, Ka, Fr = 16, 256, 4096, 768, 125
M = B * S
g = torch.Generator(device=dev).manual_seed(0)
rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)
dqkv, wqkv_t = rn(M, 3 * d) * 0.01, rn(d, 3 * d) * 0.02
dxn, resid, w, dres = rn(M, d) * 0.01, rn(M, d), rn(d), rn(M, d) * 0.01
rstd = torch.rand(M, device=dev) + 0.5
dx = rn(B, S, d) * 0.01
Xa, Xv = rn(B * S, Ka), rn(B * Fr, Ka)
da, dv = torch.empty(B, S, d, device=dev, dtype=bf), torch.empty(B, Fr, d, device=dev, dtype=bf)
gWa, gba, gWv, gbv = (torch.empty(d, Ka, device=dev), torch.empty(d, device=dev), torch.empty(d, Ka, device=dev), torch.empty(d, device=dev))
out = torch.empty(M, d, device=dev, dtype=bf)
dt3, at3 = rn(M, 192) * 0.01, rn(d, 192) * 0.02            # the engine's layout: three 64-column slices of one matrix each
dtq, atq = [dt3[:, 64 * j:64 * j + 64] for j in range(3)], [at3[:, 64 * j:64 * j + 64] for j in range(3)]
n_lora, n_conn = 32 * 16 * 8 * d, 2 * (d * Ka + d)
lp, lg, lm, lv = (torch.randn(n_lora, device=dev) * 0.01 for _ in range(4))
cp, cg, cm, cv = (torch.randn(n_conn, device=dev) * 0.01 for _ in range(4))
lv.abs_(); cv.abs_()
sumsq, parts = torch.zeros(1, device=dev), torch.zeros(1024, device=dev)
w_img, b_img = torch.empty(d, Ka, device=dev, dtype=bf), torch.empty(d, device=dev, dtype=bf)
segs, off = [], 0
for n_, wd in ((d * Ka, 0.01), (d, 0.0), (d * Ka, 0.01), (d, 0.0)):
    segs.append((cp[off:off + n_], cg[off:off + n_], cm[off:off + n_], cv[off:off + n_], wd))
    off += n_
segs.append((lp, lg, lm, lv, 0.01))


def refresh():
    lib = L.load()
    for _ in range(2):
        L.check(lib.avllm_cast(L.ptr(cp), L.F32, L.ptr(w_img), L.BF16, d * Ka, L.stream_ptr()))
        L.check(lib.avllm_cast(L.ptr(cp), L.F32, L.ptr(b_img), L.BF16, d, L.stream_ptr()))


rows = [
    ("layer-0 dX GEMM  dqkv[4096,12288] . Wqkv", lambda: ops.gemm(dqkv, wqkv_t, out=out)),
    ("layer-0 masked adapter input gradient (q,k,v)", lambda: ops.lora_dx_masked(dtq, atq, [1, 2, 3], 16, 0.05, R=out, out=out)),
    ("layer-0 input-RMSNorm backward", lambda: ops.rmsnorm_bwd(dxn, resid, w, rstd, dres=dres)),
    ("fuse_pool_bwd  [16,256,4096] -> da, dv", lambda: ops.fuse_pool_bwd(dx, S, Fr, 32, S, 0.5, da=da, dv=dv)),
    ("gemm_wgrad audio  M=4096 N=4096 K=768 (+db)", lambda: ops.gemm_wgrad(da.view(-1, d), Xa, dW=gWa, db=gba)),
    ("gemm_wgrad video  M=2000 N=4096 K=768 (+db)", lambda: ops.gemm_wgrad(dv.view(-1, d), Xv, dW=gWv, db=gbv)),
]
rows.append(("refresh of the bf16 operand images (4 casts)", refresh))
total = 0.0
for name, fn in rows:
    t = timed(fn)
    total += t
    print(f"{name:<48s} {t:8.1f} us")
opt_on = timed(lambda: ops.grad_sumsq_multi([cg, lg], sumsq, parts)) + timed(lambda: ops.adamw_step_multi(segs, 1e-5, 3, sumsq=sumsq, max_norm=0.5))
opt_off = timed(lambda: ops.grad_sumsq(lg, sumsq, partials=parts)) + timed(lambda: ops.adamw_step(lp, lg, lm, lv, 1e-5, 3, sumsq=sumsq, max_norm=0.5))
print(f"{'norm + AdamW, connector + LoRA buffers (flag on)':<48s} {opt_on:8.1f} us")
print(f"{'norm + AdamW, LoRA buffer alone (flag off)':<48s} {opt_off:8.1f} us")
print(f"{'  added by the flag':<48s} {opt_on - opt_off:8.1f} us")
total += opt_on - opt_off
print(f"{'sum of what the flag adds to a step':<48s} {total:8.1f} us   (derived estimate 450 us; accepted up to 1350 us)")
dY = da.view(-1, d)
for rep in range(3):
    ours = timed(lambda: ops.gemm_wgrad(dY, Xa, dW=gWa, want_db=False))
    theirs = timed(lambda: torch.matmul(dY.t(), Xa))
    print(f"yardstick {rep}: avllm_gemm_wgrad (fp32 out, no db) {ours:7.1f} us   torch dY.t() @ X (bf16 out) {theirs:7.1f} us")
