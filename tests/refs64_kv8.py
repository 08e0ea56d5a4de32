"""Float64 restatement of the Llama token step over an fp8 KV cache (csrc/kv_fp8.hip, ClipWhisperModel(kv_cache="fp8")): the layer arithmetic of
oracle.avsr_oracle.llama_hidden, with every cache row STORED by the OCP MX rule (e4m3 codes, one power-of-two scale per 32 consecutive elements
of a head) and read back, the token's own row included.  llama_hidden(past=...) cannot say that: it attends over the k and v it has just computed.

  * the prefill (a layer's cache is empty) attends over the pass's own k and v and only its append stores: its hidden states are those of a run
    without the option;
  * a later call stores its k (after the head norm, where the weights have one, and RoPE) and v first and attends over nothing but stored rows.

`store` is the storage: mx_store (the rule), or identity (then this file is llama_hidden with a cache; tests/test_kv8_refs_cpu.py compares them).
Plain weights only (HF names, float tensors; projection biases under `<module>.bias` where the model has them), adapters as the oracle's
`layers.N.<module>.lora_A|B` dict.  The quantiser is restated here in float64 from the rule's text, not taken from oracle/mxfp8.py, and the
same CPU file shows the two agree.  tests/test_token_step_cases_cpu.py ties the bias and head-norm terms to stored transformers logits and uses
`rnd` / `wrong` of llama_hidden (a model of the bf16 engine's roundings; planted defects) to state what the GPU bars can and cannot tell."""
import torch

from oracle import avsr_oracle as O

F64 = torch.float64
BLOCK, E4M3_MAX, E4M3_EMAX, E4M3_EMIN = 32, 448.0, 8, -6


def mx_quantize64(x):
    """x [..., K] (K % 32 == 0) -> (codes uint8 [..., K], exponents int32 [..., K/32]).  e = floor(log2 amax) - 8 clamped to [-127, 127], -127 for
    amax == 0; codes = x * 2^-e rounded to the nearest e4m3 value, ties to the even mantissa, saturated to +-448."""
    xb = x.to(F64).reshape(*x.shape[:-1], x.shape[-1] // BLOCK, BLOCK)
    amax = xb.abs().amax(-1)
    _, ex = torch.frexp(amax)                                    # amax = m 2^ex with m in [0.5, 1): floor(log2 amax) = ex - 1
    e = torch.where(amax > 0, ex.to(torch.int32) - 1 - E4M3_EMAX, torch.full_like(ex, -127, dtype=torch.int32)).clamp(-127, 127)
    y = torch.ldexp(xb, -e.unsqueeze(-1)).clamp(-E4M3_MAX, E4M3_MAX)
    _, ey = torch.frexp(y.abs())
    step = torch.ldexp(torch.ones((), dtype=F64), (ey - 1).clamp_min(E4M3_EMIN) - 3)      # 3 mantissa bits; below 2^-6 the subnormal step 2^-9
    q = torch.round(y / step) * step                             # torch.round: half to even
    return q.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8).reshape(x.shape), e


def mx_dequantize64(codes, e):
    v = codes.view(torch.float8_e4m3fn).to(F64).reshape(*codes.shape[:-1], codes.shape[-1] // BLOCK, BLOCK)
    return torch.ldexp(v, e.unsqueeze(-1)).reshape(codes.shape)


def mx_store(x):
    """What a cache row holds after it was stored and read back, float64."""
    return mx_dequantize64(*mx_quantize64(x))


def identity(x):
    return x


def _d(t):
    return t.to(F64)


def round_bf16(x):
    """A value as a bf16 tensor holds it (round to nearest even), float64: the `rnd` of llama_hidden for the bf16 engine's stored tensors."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def _lin(x, sd, lora, wkey, lkey, scale):
    y = x @ _d(sd[wkey]).T
    bkey = wkey[:-len("weight")] + "bias"                        # Qwen2: q, k, v; attention_bias: o as well (peft: base_layer(x) with its bias, + adapter)
    if bkey in sd:
        y = y + _d(sd[bkey])
    if lora is not None and (lkey + ".lora_A") in lora:
        y = y + scale * ((x @ _d(lora[lkey + ".lora_A"]).T) @ _d(lora[lkey + ".lora_B"]).T)
    return y


def _rms(x, w, eps):
    return _d(w) * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def llama_hidden(sd, lora, c, lc, x, past, pos0=0, store=mx_store, rnd=identity, wrong=()):
    """x [B, T, d] -> the hidden states after the final norm [B, T, d], float64.  past: list of (k, v) [B, Hkv, t, hd] per layer (None = empty),
    the STORED rows, extended in place.  Projection biases (`<module>.bias` under HF names) are added where the state dict has them.

    rnd: applied wherever the bf16 engine holds a bf16 tensor -- the normed input of a layer's projections, q|k|v after the bias, q and k after
    head norm and RoPE, the attention output, hmid, the residual stream after each add.  identity (the default): the float64 arithmetic;
    round_bf16: a float64 model of the engine's roundings, which tests/test_token_step_cases_cpu.py uses to state how far from the float64
    arithmetic a correct bf16 step may land.
    wrong: defects of the kind a token step can have, for that file's sensitivity checks only -- "kv_head_mod": query head h reads kv head
    h % Hkv instead of h // (H / Hkv); "attend_before_append": the step's own row is stored after the attention has run (with a zero row put
    at the first generated position by the caller, this is a writer that is one position late)."""
    x = _d(x)
    B, T, d = x.shape
    H, hd = c.heads, c.hidden // c.heads
    Hkv = getattr(c, "kv_heads", 0) or H
    cos, sin = O.rope_cos_sin(torch.arange(pos0, pos0 + T), hd, c.theta, tuple(getattr(c, "rope_scaling", ()) or ()))
    cos, sin = _d(cos), _d(sin)
    scale = lc.scale if lc is not None else 0.0
    for i in range(c.layers):
        L, K = f"model.layers.{i}.", f"layers.{i}."
        h = rnd(_rms(x, sd[L + "input_layernorm.weight"], c.eps))
        sp = lambda t, n: t.view(B, T, n, hd).transpose(1, 2)    # noqa: E731
        q = sp(rnd(_lin(h, sd, lora, L + "self_attn.q_proj.weight", K + "q_proj", scale)), H)
        k = sp(rnd(_lin(h, sd, lora, L + "self_attn.k_proj.weight", K + "k_proj", scale)), Hkv)
        v = sp(rnd(_lin(h, sd, lora, L + "self_attn.v_proj.weight", K + "v_proj", scale)), Hkv)
        if (L + "self_attn.q_norm.weight") in sd:                # Qwen3: per-head RMSNorm before RoPE
            q, k = _rms(q, sd[L + "self_attn.q_norm.weight"], c.eps), _rms(k, sd[L + "self_attn.k_norm.weight"], c.eps)
        q, k = rnd(O.apply_rope(q, cos, sin)), rnd(O.apply_rope(k, cos, sin))
        if past[i] is None:                                      # prefill: attends over its own k, v; the append stores
            past[i] = (store(k), store(v))
        elif "attend_before_append" in wrong:
            k, v, past[i] = past[i][0], past[i][1], (torch.cat([past[i][0], store(k)], 2), torch.cat([past[i][1], store(v)], 2))
        else:
            past[i] = (torch.cat([past[i][0], store(k)], 2), torch.cat([past[i][1], store(v)], 2))
            k, v = past[i]
        Tk = k.shape[2]
        if Hkv != H and "kv_head_mod" in wrong:
            k, v = k.repeat(1, H // Hkv, 1, 1), v.repeat(1, H // Hkv, 1, 1)
        elif Hkv != H:
            k, v = k.repeat_interleave(H // Hkv, 1), v.repeat_interleave(H // Hkv, 1)
        s = (q @ k.transpose(-1, -2)) * hd ** -0.5
        vis = torch.arange(Tk)[None, :] <= torch.arange(Tk - T, Tk)[:, None]
        a = rnd((torch.softmax(s.masked_fill(~vis, float("-inf")), -1) @ v).transpose(1, 2).reshape(B, T, d))
        x = rnd(x + _lin(a, sd, lora, L + "self_attn.o_proj.weight", K + "o_proj", scale))
        h = rnd(_rms(x, sd[L + "post_attention_layernorm.weight"], c.eps))
        g, u = h @ _d(sd[L + "mlp.gate_proj.weight"]).T, h @ _d(sd[L + "mlp.up_proj.weight"]).T
        x = rnd(x + rnd(torch.nn.functional.silu(g) * u) @ _d(sd[L + "mlp.down_proj.weight"]).T)
    return _rms(x, sd["model.norm.weight"], c.eps)


def step_fn(sd, lora, c, lc, x, nb=1, store=mx_store, log=None, sd_steps=None):
    """generate_ref's step(tokens, beam_idx) on this file's llama_hidden: tokens None -> the prefill logits [B * nb, V] (an item's beams repeated),
    else the cache rows reordered by beam_idx and one token per row.  log: a list that receives every step's logits.  sd_steps: the weights of
    the token steps where they are not the prefill's (decode_weights="fp8": the dequantised images)."""
    past = [None] * c.layers
    sd_p, sd = sd, (sd if sd_steps is None else sd_steps)
    state = {"pos": x.shape[1]}

    def step(tokens, beam_idx):
        with torch.no_grad():
            if tokens is None:
                h = llama_hidden(sd_p, lora, c, lc, x.repeat_interleave(nb, 0), past, 0, store)
                logits = h[:, -1] @ _d(sd_p["lm_head.weight"]).T
            else:
                for i in range(c.layers):
                    past[i] = (past[i][0].index_select(0, beam_idx), past[i][1].index_select(0, beam_idx))
                h = llama_hidden(sd, lora, c, lc, sd["model.embed_tokens.weight"][tokens][:, None], past, state["pos"], store)
                state["pos"] += 1
                logits = h[:, -1] @ _d(sd["lm_head.weight"]).T
            if log is not None:
                log.append(logits)
            return logits
    return step


def greedy(sd, lora, c, lc, x, n_new, eos, pad, store=mx_store, sd_steps=None):
    """generate_ref.token_loop on step_fn -> (tokens [B, L], top-2 margins of every step [B, L])."""
    import generate_ref
    log = []
    ids, _ = generate_ref.token_loop(step_fn(sd, lora, c, lc, x, 1, store, log, sd_steps), x.shape[0], n_new, eos, pad, None)
    top = torch.stack(log[:ids.shape[1]], 1).topk(2, -1).values
    return ids, top[..., 0] - top[..., 1]


def held_decisions(ids, ref, margins, thr):
    """The margin rule of tests/test_decode_gpu.py::test_generate_bf16_fused_token_step_vs_oracle_greedy: where the reference's top-2 margin is at
    least thr the token must be the reference's; at a near-tie either is accepted and the row ends there if the other one was taken.  Returns the
    number of decisions held; raises on a clear decision that was not made."""
    held = 0
    for b in range(ref.shape[0]):
        for t in range(min(ref.shape[1], ids.shape[1])):
            same = int(ids[b, t]) == int(ref[b, t])
            if float(margins[b, t]) >= thr:
                assert same, (b, t, ids[b].tolist(), ref[b].tolist(), margins[b].tolist())
                held += 1
            elif not same:
                break
    return held


def forced(sd, lora, c, lc, x, ids, eos, store=mx_store):
    """Teacher-forced along hypotheses ids [B, L] (each up to and including its first eos): -> (sum of the reference's log-probabilities of the
    hypothesis' tokens [B], its length [B], the reference's own top-2 margin at each of its steps, a flat list).  The cache is this file's: the
    prefill attends over its own rows, every later token over stored rows."""
    step = step_fn(sd, lora, c, lc, x, 1, store)
    B = x.shape[0]
    tot, lens, margins = torch.zeros(B, dtype=F64), torch.zeros(B, dtype=torch.int64), []
    logits = step(None, None)
    for j in range(ids.shape[1]):
        lp = torch.log_softmax(logits, -1)
        top = logits.topk(2, -1).values
        for b in range(B):
            if j == 0 or (lens[b] == j and int(ids[b, j - 1]) != eos):
                tot[b] += lp[b, int(ids[b, j])]
                lens[b] = j + 1
                margins.append(float(top[b, 0] - top[b, 1]))
        if j + 1 < ids.shape[1]:
            logits = step(ids[:, j].clamp(0, c.vocab - 1), torch.arange(B))
    return tot, lens, margins
