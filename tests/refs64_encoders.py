"""Float64 restatements of the two encoder forwards (csrc/engine.hip avllm_whisper_encoder_fwd, avllm_clip_vision_cls_fwd): the HuggingFace
arithmetic that oracle/avsr_oracle.py whisper_encoder / clip_vision_cls cite (HF modeling_whisper.py:592-646, modeling_clip.py:641-656 and the
CLS pick without post_layernorm), in float64 throughout, pure CPU.  tests/test_encoder_cases_cpu.py ties both to the oracle and to the tiny
model's golden fixtures; tests/test_encoder_matrix_gpu.py holds the engines to them.

whisper(sd, cfg, mel) -> [B, n_ctx, d];  clip_cls(sd, cfg, frames) -> [N, d].  want=True: (output, {name: tensor}) with every stored
intermediate: "conv1" (Whisper), "stem", and per block i "qkv.i", "att.i", "x_att.i" (x after attention) and "x_mlp.i" (x after the MLP; of
CLIP's last block the CLS rows only, as the engine finishes it on them).

rounded=True rounds to bf16 exactly where the bf16 engine stores bf16.  It restates the reference with the engine's STORES, not the kernels'
summation order (accumulators, softmax weights and norm statistics stay float64).  The store points, read from encoder_layers and the two
entry points:
  Whisper  the mel as im2col1_kernel<bf16> writes it into cols1; h1 = GELU(conv1 + bias); x = GELU(conv2 + bias) + pos;
           the output of the final LayerNorm;
  CLIP     the frames as patchify_kernel<bf16> writes them into cols; the patch rows patch_w cols + pos[1 + j] and the CLS rows
           class_emb + pos[0] (both into xn); x = pre_layrnorm(xn);
  a block  xn = LN1(x); qkv after the bias; att; x1 = x + out_proj(att) + bias; xn = LN2(x1); ff = act(fc1 + bias); x = x1 + fc2(ff) + bias
           (CLIP's last block: the same on the CLS rows, into xc, xcn and cls_out).
fp8= runs the four frozen projections of a block through the MX fake quantisation (oracle/mxfp8.py, as tests/refs64_fp8.py pins it); CLIP's
last block keeps out_proj / fc1 / fc2 unquantised, as the oracle states.  The engine is then the bf16 one, so the stores above are rounded
unless rounded=False says otherwise (the oracle's fp8 mode: float activations, each rounded to bf16 only on its way into a quantiser).
Each quantised input is read either before or after its bf16 store, and both are admissible: fp8="fused" quantises the unrounded LayerNorm /
attention / fc1 output (norm_mxq_kernel, the attention and fc1 epilogues), fp8="unfused" its bf16 rounding (F8_UNFUSED_QUANT=1, and whatever
shape takes no fused form); a dict {"nq": bool, "att_q": bool, "ff_q": bool} picks per input as encoder_cases.forms() names them.

wrong= plants one defect (tests/test_encoder_cases_cpu.py, "sensitivity"); the names are listed at DEFECTS."""
import torch

import refs64 as R64
from refs64_kv8 import round_bf16

F64 = torch.float64
ACT_GELU, ACT_QUICK_GELU = 1, 2
WHISPER_EPS = 1e-5                                               # engine.hip: encoder_layers(..., 1e-5f, AV_ACT_GELU, ...) and the final av_layernorm

DEFECTS = ("pos_global_row",          # the position row taken by global row index, not % n_ctx (% np): items past the first read beyond the table (zeros here)
           "cls_pos_to_patch0",       # CLIP: position row 0, the CLS one, given to patch 0 (rows 1.. shifted down by one)
           "k_bias",                  # Whisper: a k bias that is not zero (q's bias in its place)
           "conv2_phase",             # Whisper: conv2 reads t = 2 t' + kw instead of 2 t' + kw - 1
           "conv1_edge",              # Whisper: t = -1 and t = 2 n_ctx of conv1 read the neighbouring column instead of zero
           "cls_prev_frame",          # CLIP: the CLS-only block reads frame n's att and x rows from frame n - 1
           "eps_other",               # the other tower's eps (Whisper: 1e-6; CLIP: 1e-5 <-> 1e-6)
           "act_swapped",             # GELU and QuickGELU exchanged
           "pad_nan",                 # the K padding columns of cols1 / cols hold what a dirty workspace held (NaN) instead of zero
           "last_chunk_offset",       # CLIP chunk_frames: the ragged last chunk written at (chunks before it) x (its own size)
           "bf16_frames_as_fp32",     # CLIP: bf16 frames read as the halves of fp32 words
           "fp8_last_block")          # CLIP in fp8 form: out_proj / fc1 / fc2 of the CLS-only last block quantised like the others


def _d(t):
    return t.detach().to("cpu").to(F64)


def fq(x):
    """The value an e4m3 code with its block's E8M0 scale stands for (blocks of 32 along the last axis), of float64 x.  The decision is
    mxfp8.quantize's on the fp32 rounding of x; the result is exact in every format."""
    from oracle import mxfp8
    return mxfp8.fake_quant(x.to(torch.float32)).to(F64)


def _fp8_forms(fp8):
    if fp8 is None:
        return None
    if isinstance(fp8, str):
        assert fp8 in ("fused", "unfused"), fp8
        return dict.fromkeys(("nq", "att_q", "ff_q"), fp8 == "fused")
    return {k: bool(fp8[k]) for k in ("nq", "att_q", "ff_q")}


def _linear(x_exact, x_stored, w, b, quant, fused):
    """x W^T + b.  quant: through the fake quantisation, reading the unrounded input (fused) or the stored one."""
    if quant:
        return fq(x_exact if fused else round_bf16(x_stored)) @ fq(w).T + b
    return x_stored @ w.T + b


def _attention(qkv, items, T, H, scale):
    """softmax(q k^T scale) v per item and head on fused [q | k | v] rows [items * T, 3 d] -> [items * T, d]."""
    d = qkv.shape[1] // 3
    hd = d // H
    q, k, v = (t.reshape(items, T, H, hd).transpose(1, 2) for t in qkv.split(d, -1))
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    return (p @ v).transpose(1, 2).reshape(items * T, d)


def _blocks(sd, fmt, names, layers, x, items, T, H, eps, act, rnd, f8, cls_only_last, keep, wrong):
    """The pre-LN blocks on token-major x [items * T, d].  Returns x, or with cls_only_last the [items, d] CLS rows of the last block."""
    d = x.shape[1]
    hd = d // H
    out = x
    for i in range(layers):
        p = fmt.format(i)
        g = lambda k: _d(sd[p + k])                                              # noqa: E731
        last = cls_only_last and i == layers - 1
        q8 = f8 is not None                                                      # qkv is quantised in every block
        t8 = f8 is not None and (not last or "fp8_last_block" in wrong)         # the tail of CLIP's last block is not
        f = f8 or {"nq": False, "att_q": False, "ff_q": False}
        h = R64.layernorm(x, g(names["ln1"] + ".weight"), g(names["ln1"] + ".bias"), eps)
        wq, wk, wv = (g(names[n] + ".weight") for n in "qkv")
        bq, bv = g(names["q"] + ".bias"), g(names["v"] + ".bias")
        bk = _d(sd[p + names["k"] + ".bias"]) if p + names["k"] + ".bias" in sd else torch.zeros(d, dtype=F64)
        if "k_bias" in wrong:
            bk = bq
        qkv = rnd(_linear(h, rnd(h), torch.cat([wq, wk, wv], 0), torch.cat([bq, bk, bv], 0), q8, f["nq"]))
        a = _attention(qkv, items, T, H, hd ** -0.5)
        a_st = rnd(a)
        keep[f"qkv.{i}"], keep[f"att.{i}"] = qkv, a_st
        if last:                                                                 # rows n * T of att and x: the CLS rows
            idx = torch.arange(items) * T
            if "cls_prev_frame" in wrong:
                idx = (torch.arange(items) - 1).clamp_min(0) * T
            a, a_st, x = a[idx], a_st[idx], x[idx]
        x1 = rnd(x + _linear(a, a_st, g(names["o"] + ".weight"), g(names["o"] + ".bias"), t8, f["att_q"]))
        h = R64.layernorm(x1, g(names["ln2"] + ".weight"), g(names["ln2"] + ".bias"), eps)
        z = R64.activation(_linear(h, rnd(h), g(names["fc1"] + ".weight"), g(names["fc1"] + ".bias"), t8, f["nq"]), act)
        x = rnd(x1 + _linear(z, rnd(z), g(names["fc2"] + ".weight"), g(names["fc2"] + ".bias"), t8, f["ff_q"]))
        keep[f"x_att.{i}"], keep[f"x_mlp.{i}"] = x1, x
        out = x
    return out


def _setup(rounded, fp8, wrong):
    f8 = _fp8_forms(fp8)
    assert all(w in DEFECTS for w in wrong), wrong
    if rounded is None:
        rounded = f8 is not None
    rnd = round_bf16 if rounded else (lambda t: t)
    return f8, rnd


WHISPER_NAMES = dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.out_proj",
                     ln1="self_attn_layer_norm", ln2="final_layer_norm", fc1="fc1", fc2="fc2")
CLIP_NAMES = dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.out_proj",
                  ln1="layer_norm1", ln2="layer_norm2", fc1="mlp.fc1", fc2="mlp.fc2")


def whisper(sd, cfg, mel, rounded=None, fp8=None, want=False, wrong=()):
    if mel.dim() != 3 or mel.shape[1] != cfg.n_mels or mel.shape[-1] != 2 * cfg.n_ctx:
        raise ValueError(f"Whisper expects the mel input features to be [B, {cfg.n_mels}, {2 * cfg.n_ctx}], but found {tuple(mel.shape)}")
    f8, rnd = _setup(rounded, fp8, wrong)
    B, C, T2 = mel.shape
    d, n_ctx = cfg.d_model, cfg.n_ctx
    act = ACT_QUICK_GELU if "act_swapped" in wrong else ACT_GELU
    eps = 1e-6 if "eps_other" in wrong else WHISPER_EPS
    keep = {}
    # conv1 (k 3, padding 1): h1[b, t, o] = GELU(b1[o] + sum_{c, kw} w1[o, c, kw] mel[b, c, t + kw - 1]), zero beyond the edges
    m = rnd(_d(mel)).transpose(1, 2)                                             # [B, T2, C]
    lo, hi = (m[:, 1:2], m[:, -2:-1]) if "conv1_edge" in wrong else (torch.zeros(B, 1, C, dtype=F64),) * 2
    mp = torch.cat([lo, m, hi], 1)
    cols1 = torch.stack([mp[:, kw:kw + T2] for kw in range(3)], -1).reshape(B * T2, 3 * C)          # column c * 3 + kw
    z1 = cols1 @ _d(sd["encoder.conv1.weight"]).reshape(d, 3 * C).T + _d(sd["encoder.conv1.bias"])
    if "pad_nan" in wrong and (3 * C) % 64:
        z1 = z1 + float("nan") * 0.0
    h1 = rnd(R64.activation(z1, act)).reshape(B, T2, d)
    keep["conv1"] = h1
    # conv2 (k 3, stride 2, padding 1): reads h1[b, 2 t' + kw - 1]
    hp = torch.cat([torch.zeros(B, 1, d, dtype=F64), h1, torch.zeros(B, 2, d, dtype=F64)], 1)
    off = 1 if "conv2_phase" in wrong else 0
    cols2 = torch.cat([hp[:, off + kw:off + kw + T2:2] for kw in range(3)], -1).reshape(B * n_ctx, 3 * d)      # column kw * d + c
    z2 = cols2 @ _d(sd["encoder.conv2.weight"]).permute(0, 2, 1).reshape(d, 3 * d).T + _d(sd["encoder.conv2.bias"])
    pos = _d(sd["encoder.embed_positions.weight"])
    if "pos_global_row" in wrong:
        pos_rows = torch.cat([pos, torch.zeros((B - 1) * n_ctx, d, dtype=F64)], 0)
    else:
        pos_rows = pos.repeat(B, 1)
    x = rnd(R64.activation(z2, act) + pos_rows)
    keep["stem"] = x.reshape(B, n_ctx, d)
    x = _blocks(sd, "encoder.layers.{}.", WHISPER_NAMES, cfg.layers, x, B, n_ctx, cfg.heads, eps, act, rnd, f8, False, keep, wrong)
    out = rnd(R64.layernorm(x, _d(sd["encoder.layer_norm.weight"]), _d(sd["encoder.layer_norm.bias"]), eps)).reshape(B, n_ctx, d)
    return (out, keep) if want else out


def frames_as_fp32_halves(frames):
    """What a kernel reading bf16 frames as fp32 words sees: two bf16 values per word, the first half of the words from the buffer and the
    rest, past its end, taken as zero."""
    raw = frames.to(torch.bfloat16).contiguous().view(torch.int16).flatten()
    n = raw.numel()
    words = torch.cat([raw, raw.new_zeros(n % 2)]).view(torch.float32)
    return torch.cat([words, torch.zeros(n - words.numel())]).reshape(frames.shape)


def clip_cls(sd, cfg, frames, rounded=None, fp8=None, want=False, wrong=(), chunk=0):
    sd = {k[len("vision_model."):] if k.startswith("vision_model.") else k: v for k, v in sd.items()}
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[-1] != cfg.image or frames.shape[-2] != cfg.image:
        raise ValueError(f"Input image size {tuple(frames.shape)} doesn't match model ({cfg.image}*{cfg.image}).")
    if cfg.layers < 1:
        raise ValueError("clip_cls: the CLS rows come out of the last block: layers >= 1")
    f8, rnd = _setup(rounded, fp8, wrong)
    N, p, d = frames.shape[0], cfg.patch, cfg.hidden
    g = cfg.image // p
    np_, T = g * g, g * g + 1
    act = ACT_GELU if "act_swapped" in wrong else ACT_QUICK_GELU
    eps = ({1e-5: 1e-6, 1e-6: 1e-5}[cfg.eps]) if "eps_other" in wrong else cfg.eps
    keep = {}
    fr = frames_as_fp32_halves(frames) if "bf16_frames_as_fp32" in wrong else frames
    fr = rnd(_d(fr))
    # patch (py, px) of frame n -> row n * np + py * g + px, column c * p * p + ky * p + kx: Conv2d(kernel p, stride p, no bias)
    cols = fr.reshape(N, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(N * np_, 3 * p * p)
    pe = cols @ _d(sd["embeddings.patch_embedding.weight"]).reshape(d, 3 * p * p).T
    if "pad_nan" in wrong and (3 * p * p) % 64:
        pe = pe + float("nan") * 0.0
    pos = _d(sd["embeddings.position_embedding.weight"])
    if "pos_global_row" in wrong:
        patch_pos = torch.cat([pos[1:], torch.zeros((N - 1) * np_, d, dtype=F64)], 0)
    elif "cls_pos_to_patch0" in wrong:
        patch_pos = pos[:np_].repeat(N, 1)
    else:
        patch_pos = pos[1:].repeat(N, 1)
    x = torch.empty(N, T, d, dtype=F64)
    x[:, 1:] = rnd(pe + patch_pos).reshape(N, np_, d)
    x[:, 0] = rnd(_d(sd["embeddings.class_embedding"]) + pos[0])
    x = rnd(R64.layernorm(x.reshape(N * T, d), _d(sd["pre_layrnorm.weight"]), _d(sd["pre_layrnorm.bias"]), eps))
    keep["stem"] = x.reshape(N, T, d)
    out = _blocks(sd, "encoder.layers.{}.", CLIP_NAMES, cfg.layers, x, N, T, cfg.heads, eps, act, rnd, f8, True, keep, wrong)
    if "last_chunk_offset" in wrong and chunk and chunk < N and N % chunk:
        n_last, before = N % chunk, N // chunk
        moved = out.clone()
        moved[N - n_last:] = 0.0                                                 # never written
        moved[before * n_last:before * n_last + n_last] = out[N - n_last:]
        out = moved
    return (out, keep) if want else out
