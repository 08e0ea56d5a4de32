#!/usr/bin/env python3
"""What LoRA adapters on gate_proj / up_proj / down_proj cost (lora_target_modules="all-linear" against the default q, k, v, o), at Llama-2-7B
shapes with synthetic weights, bf16.

  * the LLM half of the train step (avllm_llama_lora_fwd_loss + _bwd) at B = 16, S = 256, lora_dropout 0.05: default targets against
    all-linear, two engines in one process alternated round by round, hipEvent timing, median of the rounds and their spread (max - min);
  * the token step at batch 8 with the all-linear adapters attached (the general step: an unmerged MLP adapter leaves the fused path) against
    the same engine after merge_lora() (the fused step), both as plain host-driven calls of decode_step at cache position 300;
  * the two launch forms of the gate|up adapter term in the forward: one N = 2 ffn GEMM whose second K segment is a
    block-diagonal [2 ffn, 128] image of B_gate and B_up, against two N = ffn GEMMs with a 64-wide second K segment each.

--layers N builds fewer decoder layers than the model's 32 (the step scales with the layer count; lm_head and the loss do not)."""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "audio-visual-llm_amd"))
import torch
from avllm import ops
from avllm.arch import LORA_DEFAULT_TARGETS, LORA_MODULES, LlamaCfg, LoraCfg
from avllm.engine import LlamaEngine

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--seq", type=int, default=256)
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--dropout", type=float, default=0.05)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=3, help="train steps per round")
ap.add_argument("--token-steps", type=int, default=30)
ap.add_argument("--token-batch", type=int, default=8)
a = ap.parse_args()
dev, BF = "cuda:0", torch.bfloat16
cfg = LlamaCfg(4096, 32, a.layers, 11008, 32000)
d, f = cfg.hidden, cfg.ffn
g = torch.Generator(device=dev).manual_seed(0)
med = statistics.median


def w(o, k):
    return torch.randn(o, k, device=dev, generator=g, dtype=BF) * k ** -0.5


def timed(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def report(name, res):
    return f"{name} {med(res):.3f} ms +-{max(res) - min(res):.3f}"


sd = {"model.embed_tokens.weight": w(cfg.vocab, d), "model.norm.weight": torch.ones(d, device=dev, dtype=BF), "lm_head.weight": w(cfg.vocab, d)}
for i in range(cfg.layers):
    p = f"model.layers.{i}."
    for nm, (o, k) in {"self_attn.q_proj": (d, d), "self_attn.k_proj": (d, d), "self_attn.v_proj": (d, d), "self_attn.o_proj": (d, d),
                       "mlp.gate_proj": (f, d), "mlp.up_proj": (f, d), "mlp.down_proj": (d, f)}.items():
        sd[p + nm + ".weight"] = w(o, k)
    sd[p + "input_layernorm.weight"] = torch.ones(d, device=dev, dtype=BF)
    sd[p + "post_attention_layernorm.weight"] = torch.ones(d, device=dev, dtype=BF)


def engine(targets, training):
    eng = LlamaEngine(sd, cfg, LoraCfg(a.rank, 2.0 * a.rank, targets), None, dtype=BF, device=dev, training=training)
    eng.lora_p.copy_(torch.randn(eng.lora_p.shape, device=dev, generator=g) * 0.01)
    eng.pack_lora()
    return eng


# ---- train step
B, S = a.batch, a.seq
x = torch.randn(B, S, d, device=dev, generator=g, dtype=BF) * 0.5
labels = torch.randint(3, cfg.vocab, (B, S), device=dev, generator=g)
legs = {"default": engine(LORA_DEFAULT_TARGETS, True), "all-linear": engine(LORA_MODULES, True)}
seed = [0]


def train_step(eng):
    seed[0] += 1
    eng.fwd_loss(x, labels, dropout=a.dropout, seed=seed[0])
    eng.lora_g.zero_()
    eng.bwd()


for eng in legs.values():
    train_step(eng)                                   # sizes the workspace, loads the code objects
res = {n: [] for n in legs}
for _ in range(a.rounds):
    for n, eng in legs.items():
        res[n].append(timed(lambda: train_step(eng), a.steps))
print(f"llama2-7b shapes, {cfg.layers} layers, rank {a.rank}, bf16, B={B} S={S}, lora_dropout {a.dropout}; LLM half of the train step (fwd_loss + bwd): "
      + "  ".join(report(n, res[n]) for n in legs) + f"  all-linear/default {med(res['all-linear']) / med(res['default']):.3f}x"
      + f"  trainable parameters {legs['default'].lora_p.numel() / 1e6:.1f} M -> {legs['all-linear'].lora_p.numel() / 1e6:.1f} M"
      + "  rounds " + " ".join(f"{n} {[round(t, 2) for t in res[n]]}" for n in legs), flush=True)
del legs
torch.cuda.empty_cache()

# ---- token step: adapters attached (general step) against merged (fused step)
Bt = a.token_batch
eng = engine(LORA_MODULES, False)
ids = torch.randint(0, cfg.vocab, (Bt,), device=dev, generator=g)
out = torch.empty(Bt, cfg.vocab, device=dev, dtype=torch.float32)


def token_leg():
    kc, vc = eng.alloc_cache(Bt, 320 + a.token_steps + 8)
    pos = [300]

    def one():
        eng.decode_step(ids, pos[0], kc, vc, logits=out)
        pos[0] += 1
    one()
    r = []
    for _ in range(a.rounds):
        pos[0] = 300
        r.append(timed(one, a.token_steps))
    return r


assert not eng.decode_is_fused(Bt)
t_un = token_leg()
eng.merge_lora()
assert eng.decode_is_fused(Bt)
t_me = token_leg()
print(f"token step, batch {Bt}, cache position 300, host-driven decode_step: {report('all-linear adapters attached (general step)', t_un)}  "
      f"{report('merged (fused step)', t_me)}  attached/merged {med(t_un) / med(t_me):.2f}x", flush=True)
del eng
torch.cuda.empty_cache()

# ---- the two launch forms of the gate|up adapter term
M = B * S
xn = torch.randn(M, d, device=dev, generator=g, dtype=BF)
wgu = w(2 * f, d)
t2 = torch.zeros(M, 128, device=dev, dtype=BF)
t2[:, :a.rank] = torch.randn(M, a.rank, device=dev, generator=g, dtype=BF)
t2[:, 64:64 + a.rank] = torch.randn(M, a.rank, device=dev, generator=g, dtype=BF)
bd = torch.zeros(2 * f, 128, device=dev, dtype=BF)                       # block diagonal: gate's rows read columns 0..63, up's 64..127
bg, bu = torch.zeros(f, 64, device=dev, dtype=BF), torch.zeros(f, 64, device=dev, dtype=BF)
bg[:, :a.rank] = torch.randn(f, a.rank, device=dev, generator=g, dtype=BF) * 0.1
bu[:, :a.rank] = torch.randn(f, a.rank, device=dev, generator=g, dtype=BF) * 0.1
bd[:f, :64], bd[f:, 64:] = bg, bu
gu1, gu2 = torch.empty(M, 2 * f, device=dev, dtype=BF), torch.empty(M, 2 * f, device=dev, dtype=BF)


def one_gemm():
    ops.gemm(xn, wgu, out=gu1, A2=t2, B2=bd)


def two_gemms():
    ops.gemm(xn, wgu[:f], out=gu2[:, :f], A2=t2[:, :64], B2=bg)
    ops.gemm(xn, wgu[f:], out=gu2[:, f:], A2=t2[:, 64:], B2=bu)


def plain():
    ops.gemm(xn, wgu, out=gu1)


plain(); one_gemm(); two_gemms()
same = float((gu1.float() - gu2.float()).abs().max())
r1, r2, r0 = [], [], []
for _ in range(a.rounds):
    r0.append(timed(plain, 10)); r1.append(timed(one_gemm, 10)); r2.append(timed(two_gemms, 10))
print(f"gate|up projection with its adapter term, M={M} d={d} ffn={f}: {report('frozen product alone (N = 2 ffn)', r0)}  "
      f"{report('one N = 2 ffn GEMM, block-diagonal K2 = 128', r1)}  {report('two N = ffn GEMMs, K2 = 64 each', r2)}  "
      f"two/one {med(r2) / med(r1):.3f}x  (max |difference| of the two results {same:.3g})", flush=True)
