"""Host-side owners of device weights/workspaces for the three model-level C-ABI engines.

Weights arrive as HuggingFace-named state dicts (the modules the reference instantiates:
clip_whisper_model.py:864-1019), are re-laid-out once for the HIP kernels (fused qkv / gate-up, im2col-ordered
conv weights, transposed images for the dX GEMMs) and stay resident in HBM.  All compute is in libavllm.so.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import lib as L
from . import ops
from .arch import LORA_MLP_MODULES, LORA_MODULES, check_llama_keys, lora_layout, lora_shapes


class Workspace:
    """One growable byte buffer handed to the C ABI as scratch (the library never allocates).

    `Workspace.generation` counts reallocations of ANY workspace: a captured hipGraph holds raw pointers into these buffers, so whoever
    replays one compares the generation it captured under with the current one and drops its graphs when they differ
    (ClipWhisperTrainer.train_step).  Growth is monotonic, so a mix of input signatures settles after each has been seen once."""

    generation = 0

    def __init__(self, device):
        self.device = device
        self.buf = None

    def get(self, nbytes: int):
        if self.buf is None or self.buf.numel() < nbytes:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("workspace would grow inside a hipGraph capture (the eager warm-up step must size it first)")
            self.buf = None
            self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            Workspace.generation += 1
        return self.buf


def _dev(t, dtype, device):
    return t.detach().to(device=device, dtype=dtype).contiguous()


def _pad_cols(w2d, kpad):
    if w2d.shape[1] == kpad:
        return w2d
    out = torch.zeros(w2d.shape[0], kpad, dtype=w2d.dtype, device=w2d.device)
    out[:, : w2d.shape[1]] = w2d
    return out


def _fp8_images(w, keep):
    """Block-scaled fp8 image of a weight matrix [N,K] (weight-side layout) -> (codes ptr, scales ptr); tensors parked in `keep`."""
    q, s = ops.mx_quantize(w, 1)
    keep += [q, s]
    return q.data_ptr(), s.data_ptr()


def _enc_layers(sd, prefix_fmt, n, names, dtype, device, keep, fp8=False):
    """Build the EncLayer array for a pre-LN encoder; `names` maps our fields to HF suffixes."""
    arr = (L.EncLayer * n)()
    for i in range(n):
        p = prefix_fmt.format(i)
        g = lambda k: sd[p + k]
        q, k_, v = g(names["q"] + ".weight"), g(names["k"] + ".weight"), g(names["v"] + ".weight")
        d = q.shape[0]
        bq = g(names["q"] + ".bias")
        bk = sd.get(p + names["k"] + ".bias")
        if bk is None:
            bk = torch.zeros(d, dtype=bq.dtype, device=bq.device)     # Whisper k_proj has no bias (HF whisper :276)
        bv = g(names["v"] + ".bias")
        t = {
            "ln1_w": g(names["ln1"] + ".weight"), "ln1_b": g(names["ln1"] + ".bias"),
            "wqkv": torch.cat([q, k_, v], 0), "bqkv": torch.cat([bq, bk, bv], 0),
            "wo": g(names["o"] + ".weight"), "bo": g(names["o"] + ".bias"),
            "ln2_w": g(names["ln2"] + ".weight"), "ln2_b": g(names["ln2"] + ".bias"),
            "w1": g(names["fc1"] + ".weight"), "b1": g(names["fc1"] + ".bias"),
            "w2": g(names["fc2"] + ".weight"), "b2": g(names["fc2"] + ".bias"),
        }
        for k, val in t.items():
            dv = _dev(val, dtype, device)
            keep.append(dv)
            setattr(arr[i], k, dv.data_ptr())
            if fp8 and k in ("wqkv", "wo", "w1", "w2"):
                q8, s8 = _fp8_images(dv, keep)
                f = {"wqkv": ("wqkv8", "sqkv8"), "wo": ("wo8", "so8"), "w1": ("w18", "s18"), "w2": ("w28", "s28")}[k]
                setattr(arr[i], f[0], q8); setattr(arr[i], f[1], s8)
    return arr


class WhisperEngine:
    """avllm_whisper_encoder_fwd: mel f32 [B,80,2*n_ctx] -> [B,n_ctx,d]."""

    def __init__(self, sd, cfg, dtype=torch.bfloat16, device="cuda", fp8=False):
        self.cfg, self.dtype, self.device = cfg, dtype, device
        self.keep = []
        d = cfg.d_model
        k1pad = (3 * cfg.n_mels + 63) // 64 * 64
        w = L.Whisper()
        w.dtype, w.d, w.heads, w.layers, w.ffn, w.n_mels, w.n_ctx, w.k1pad = (
            L.F32 if dtype == torch.float32 else L.BF16, d, cfg.heads, cfg.layers, cfg.ffn, cfg.n_mels, cfg.n_ctx, k1pad)
        c1 = _pad_cols(sd["encoder.conv1.weight"].reshape(d, 3 * cfg.n_mels), k1pad)         # column c*3+kw
        c2 = sd["encoder.conv2.weight"].permute(0, 2, 1).reshape(d, 3 * d)                   # column kw*d+c
        for name, val in (("conv1_w", c1), ("conv1_b", sd["encoder.conv1.bias"]), ("conv2_w", c2),
                          ("conv2_b", sd["encoder.conv2.bias"]), ("pos", sd["encoder.embed_positions.weight"]),
                          ("lnf_w", sd["encoder.layer_norm.weight"]), ("lnf_b", sd["encoder.layer_norm.bias"])):
            dv = _dev(val, dtype, device)
            self.keep.append(dv)
            setattr(w, name, dv.data_ptr())
        names = dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.out_proj",
                     ln1="self_attn_layer_norm", ln2="final_layer_norm", fc1="fc1", fc2="fc2")
        self.layers = _enc_layers(sd, "encoder.layers.{}.", cfg.layers, names, dtype, device, self.keep, fp8)
        w.layer = C.cast(self.layers, C.POINTER(L.EncLayer))
        w.fp8 = int(bool(fp8))
        self.desc = w
        self.ws = Workspace(device)

    def forward(self, mel):
        if mel.dim() != 3 or mel.shape[1] != self.cfg.n_mels:
            raise ValueError(f"Audio input should have shape [batch_size, {self.cfg.n_mels}, time_steps], but got {tuple(mel.shape)}")
        if mel.shape[-1] != 2 * self.cfg.n_ctx:
            raise ValueError(f"Whisper expects the mel input features to be of length {2 * self.cfg.n_ctx}, but found {mel.shape[-1]}")
        lib = L.load()
        mel = mel.to(device=self.device, dtype=torch.float32).contiguous()
        B = mel.shape[0]
        out = torch.empty(B, self.cfg.n_ctx, self.cfg.d_model, device=self.device, dtype=self.dtype)
        n = lib.avllm_whisper_workspace_bytes(C.byref(self.desc), B)
        ws = self.ws.get(n)
        L.check(lib.avllm_whisper_encoder_fwd(C.byref(self.desc), L.ptr(mel), B, L.ptr(out), L.ptr(ws), ws.numel(), L.stream_ptr()))
        return out


class ClipEngine:
    """avllm_clip_vision_cls_fwd: frames f32 [N,3,S,S] -> CLS of last_hidden_state [N,d] (no post_layernorm)."""

    def __init__(self, sd, cfg, dtype=torch.bfloat16, device="cuda", chunk_frames=0, fp8=False):
        sd = {k[len("vision_model."):] if k.startswith("vision_model.") else k: v for k, v in sd.items()}
        self.cfg, self.dtype, self.device = cfg, dtype, device
        if cfg.layers < 1:      # avllm_clip_vision_cls_fwd refuses it too: the CLS rows are written by the last block
            raise ValueError(f"ClipEngine: layers={cfg.layers}: the CLS output is written by the last block, a tower without one has none")
        self.chunk = chunk_frames
        self.keep = []
        d = cfg.hidden
        kpad = (3 * cfg.patch * cfg.patch + 63) // 64 * 64
        c = L.Clip()
        c.dtype, c.d, c.heads, c.layers, c.ffn, c.image, c.patch, c.tokens = (
            L.F32 if dtype == torch.float32 else L.BF16, d, cfg.heads, cfg.layers, cfg.mlp, cfg.image, cfg.patch, cfg.tokens)
        c.eps = cfg.eps
        pw = _pad_cols(sd["embeddings.patch_embedding.weight"].reshape(d, -1), kpad)
        for name, val in (("patch_w", pw), ("class_emb", sd["embeddings.class_embedding"]),
                          ("pos", sd["embeddings.position_embedding.weight"]), ("pre_ln_w", sd["pre_layrnorm.weight"]),
                          ("pre_ln_b", sd["pre_layrnorm.bias"])):
            dv = _dev(val, dtype, device)
            self.keep.append(dv)
            setattr(c, name, dv.data_ptr())
        names = dict(q="self_attn.q_proj", k="self_attn.k_proj", v="self_attn.v_proj", o="self_attn.out_proj",
                     ln1="layer_norm1", ln2="layer_norm2", fc1="mlp.fc1", fc2="mlp.fc2")
        self.layers = _enc_layers(sd, "encoder.layers.{}.", cfg.layers, names, dtype, device, self.keep, fp8)
        c.layer = C.cast(self.layers, C.POINTER(L.EncLayer))
        c.fp8 = int(bool(fp8))
        self.desc = c
        self.ws = Workspace(device)

    def forward(self, frames):
        if frames.dim() != 4 or frames.shape[1] != 3:
            raise ValueError(f"frames should have shape [N, 3, H, W], but got {tuple(frames.shape)}")
        if frames.shape[-1] != self.cfg.image or frames.shape[-2] != self.cfg.image:
            raise ValueError(f"Input image size ({frames.shape[-2]}*{frames.shape[-1]}) doesn't match model ({self.cfg.image}*{self.cfg.image}).")
        lib = L.load()
        # fp32 pixel_values as the reference's CLIPProcessor hands them over, or bf16 (device-side preprocessing, avllm.preprocess.ClipFrames)
        frames = frames.to(device=self.device, dtype=torch.bfloat16 if frames.dtype == torch.bfloat16 else torch.float32).contiguous()
        self.desc.frames_bf16 = int(frames.dtype == torch.bfloat16)
        N = frames.shape[0]
        out = torch.empty(N, self.cfg.hidden, device=self.device, dtype=self.dtype)
        step = self.chunk if self.chunk and self.chunk < N else N
        ws = self.ws.get(lib.avllm_clip_workspace_bytes(C.byref(self.desc), step))
        for s in range(0, N, step):
            n = min(step, N - s)
            L.check(lib.avllm_clip_vision_cls_fwd(C.byref(self.desc), L.ptr(frames[s:]), n, L.ptr(out[s:]), L.ptr(ws), ws.numel(), L.stream_ptr()))
        return out


LORA_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj")


class LlamaEngine:
    """Llama + LoRA: avllm_llama_lora_fwd_loss / _bwd (training) and prefill / decode_step (generation).

    Trainable state: one flat fp32 buffer `lora_p` holding, per layer, [A_q,B_q,A_k,B_k,A_v,B_v,A_o,B_o]
    (A [r,d], B [dout,r]; dout = d, or kv_heads*head_dim for k/v under grouped-query attention) so a layer's gradient bucket is one contiguous slice of `lora_g` for the DDP all-reduce.
    `lora_cfg.targets` (arch.parse_lora_targets) selects the adapted modules out of q, k, v, o, gate, up, down: a layer's slice then holds the
    selected ones only, in that canonical order, A then B (gate, up: A [r,d], B [ffn,r]; down: A [r,ffn], B [d,r]).  The default four give the
    layout above.  An unmerged adapter on gate, up or down keeps the token step off the fused path (decode_is_fused); merge_lora() folds them.
    """

    def __init__(self, sd, cfg, lora_cfg=None, lora_sd=None, dtype=torch.bfloat16, device="cuda", training=True, fp8=False, decode_fp8=False,
                 decode_fp4=False, kv_fp8=False):
        self.cfg, self.lcfg, self.dtype, self.device, self.training = cfg, lora_cfg, dtype, device, training
        self.fp8 = bool(fp8)
        # weight-only fp8 token step (include/avllm.h avllm_llama.decode_fp8): the fused decode path streams e4m3 codes + layout-2 exponents
        self.decode_fp8 = bool(decode_fp8)
        if self.decode_fp8 and dtype != torch.bfloat16:
            raise ValueError("decode_fp8 needs the bf16 engine")
        # weight-only fp4 token step (avllm_llama.decode_fp4): the four projections of a layer stream MXFP4 codes, lm_head streams e4m3
        self.decode_fp4 = bool(decode_fp4)
        if self.decode_fp4 and (dtype != torch.bfloat16 or self.decode_fp8):
            raise ValueError("decode_fp4 needs the bf16 engine and excludes decode_fp8")
        # fp8 KV cache of generate() (avllm_llama.kv_fp8): alloc_cache() hands out block-scaled e4m3 images for the row counts the fused token
        # step takes (decode_caches_fp8); prefill() and decode_step() tell the library the form of the cache they are given
        self.kv_fp8 = bool(kv_fp8)
        if self.kv_fp8 and dtype != torch.bfloat16:
            raise ValueError("kv_fp8 needs the bf16 engine")
        self.keep = []
        d, f = cfg.hidden, cfg.ffn
        self.use_lora = lora_cfg is not None
        r = lora_cfg.r if self.use_lora else 0
        self.r = r
        # the adapted modules in canonical order (without LoRA: the default four, which only size the -- unused -- layout)
        self.targets = tuple(getattr(lora_cfg, "targets", None) or LORA_TARGETS) if self.use_lora else LORA_TARGETS
        self.mlp_targets = tuple(nm for nm in self.targets if nm in LORA_MLP_MODULES)
        if self.fp8 and self.mlp_targets:
            raise NotImplementedError(f"precision='fp8' with a LoRA adapter on {', '.join(self.mlp_targets)} is not implemented: "
                                      "the fp8 training forward takes adapters on q_proj, k_proj, v_proj and o_proj only")
        m = L.Llama()
        m.dtype, m.d, m.heads, m.layers, m.ffn, m.vocab, m.lora_r = (
            L.F32 if dtype == torch.float32 else L.BF16, d, cfg.heads, cfg.layers, f, cfg.vocab, r)
        kvh = getattr(cfg, "kv_heads", 0) or cfg.heads
        if cfg.heads % kvh:
            raise ValueError(f"heads={cfg.heads} is not a multiple of kv_heads={kvh}")
        m.kv_heads = kvh
        self.dkv = kvh * (d // cfg.heads)
        self.douts = (d, self.dkv, self.dkv, d)                  # output width of q, k, v, o (grouped-query: k/v are narrower)
        m.eps, m.theta, m.lora_scale = cfg.eps, cfg.theta, (lora_cfg.scale if self.use_lora else 0.0)
        rs = tuple(getattr(cfg, "rope_scaling", ()) or ())
        if rs:                                                   # Llama-3.1 / 3.2 "llama3" RoPE frequency scaling (include/avllm.h)
            m.rope_factor, m.rope_low_freq_factor, m.rope_high_freq_factor, m.rope_orig_ctx = float(rs[0]), float(rs[1]), float(rs[2]), int(rs[3])

        # the LLM's device tensors by their HuggingFace names (the fused q|k|v and gate|up matrices of layer i under (i, "qkv"), (i, "gu")):
        # what merge_lora() writes into and merged_llm_state_dict() exports
        self.llm_w = {}

        def put(val, name=None):
            dv = _dev(val, dtype, device)
            self.keep.append(dv)
            if name is not None:
                self.llm_w[name] = dv
            return dv

        def put_sd(name):
            return put(sd[name], name)

        self.embed = put_sd("model.embed_tokens.weight")
        m.embed = self.embed.data_ptr()
        m.norm_w = put_sd("model.norm.weight").data_ptr()
        head = put_sd("lm_head.weight")
        m.lm_head = head.data_ptr()
        if training:
            m.lm_head_t = put(head.t()).data_ptr()
        m.fp8 = int(self.fp8)

        def images(w, decode8=self.decode_fp8, key=None):
            """(codes, layout-1 image, layout-2 exponents) pointers of a frozen matrix for the fp8 modes that are on (None otherwise); the
            token step's exponents share the codes of the training forward's image when both modes are on (re-quantising writes the same bytes).
            `key`: the matrix's name in self.llm_w when merge_lora() has to rewrite its images in place."""
            q = s = e = None
            if self.fp8:
                q, s = ops.mx_quantize(w, 1)
                self.keep += [q, s]
            if decode8:
                q, e = ops.mx_quantize(w, 2, q=q)
                self.keep += [q, e]
            if key is not None:
                self.img8[key] = (q, s, e)
            return tuple(None if t is None else t.data_ptr() for t in (q, s, e))

        m.decode_fp8 = int(self.decode_fp8)
        m.decode_fp4 = int(self.decode_fp4)
        m.kv_fp8 = int(self.kv_fp8)
        if self.fp8 or self.decode_fp8 or self.decode_fp4:
            m.lm_head8, m.slm_head8, m.elm_head8 = images(head, self.decode_fp8 or self.decode_fp4)
        self.layers = (L.LlamaLayer * cfg.layers)()
        check_llama_keys(sd, cfg)
        # what else merge_lora() touches: the fp8 (codes, layout-1 image, layout-2 exponents) and fp4 (codes, exponents) images of the
        # attention matrices by (layer, "qkv" | "o"), which it rewrites, and their transposed training copies, which it frees
        self.merged = False
        self.img8, self.img4, self.attn_wt, self.mlp_wt = {}, {}, {}, {}
        # ---- LoRA masters / grads / padded operand images
        self.mod_shapes = {nm: lora_shapes(cfg, r, nm) for nm in LORA_MODULES}      # name -> ((r, din), (dout, r))
        self.per_layer, self._layout = lora_layout(cfg, r, self.targets)
        n = cfg.layers * self.per_layer
        if self.use_lora:
            self.lora_p = torch.zeros(n, dtype=torch.float32, device=device)
            self.lora_g = torch.zeros(n, dtype=torch.float32, device=device)
            P = L.LORA_PAD
            self.img_A = torch.zeros(cfg.layers, 4, P, d, dtype=dtype, device=device)
            self.img_ATqkv = torch.zeros(cfg.layers, d, 3 * P, dtype=dtype, device=device)
            self.img_ATo = torch.zeros(cfg.layers, d, P, dtype=dtype, device=device)
            self.img_B = [[torch.zeros(do, P, dtype=dtype, device=device) for do in self.douts] for _ in range(cfg.layers)]
            self.img_BT = [[torch.zeros(P, do, dtype=dtype, device=device) for do in self.douts] for _ in range(cfg.layers)]
            # gate / up / down, the selected ones only: name -> per-layer images.  gate and up share one [d, 2*64] transposed-A image when both
            # are adapted (the second K segment of the dxn product), as q, k, v share img_ATqkv
            z = lambda *shape: [torch.zeros(*shape, dtype=dtype, device=device) for _ in range(cfg.layers)]
            self.mlp_img = {}
            gu_shared = z(d, 2 * P) if "gate_proj" in self.targets and "up_proj" in self.targets else None
            for k, nm in enumerate(LORA_MLP_MODULES):
                if nm not in self.targets:
                    continue
                (_, din), (dout, _) = self.mod_shapes[nm]
                im = {"A": z(P, din), "B": z(dout, P), "BT": z(P, dout)}
                if gu_shared is not None and k < 2:
                    im["AT"], im["ld_at"], im["at_col"] = gu_shared, 2 * P, k * P
                else:
                    im["AT"], im["ld_at"], im["at_col"] = z(din, P), P, 0
                self.mlp_img[nm] = im
            if lora_sd is not None:
                self.load_lora(lora_sd)
        for i in range(cfg.layers):
            p = f"model.layers.{i}."
            ly = self.layers[i]
            wqkv = put(torch.cat([sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.k_proj.weight"],
                                  sd[p + "self_attn.v_proj.weight"]], 0), (i, "qkv"))
            wo = put_sd(p + "self_attn.o_proj.weight")
            wgu = put(torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], 0), (i, "gu"))
            wdown = put_sd(p + "mlp.down_proj.weight")
            ly.ln1_w = put_sd(p + "input_layernorm.weight").data_ptr()
            ly.ln2_w = put_sd(p + "post_attention_layernorm.weight").data_ptr()
            ly.wqkv, ly.wo, ly.wgu, ly.wdown = wqkv.data_ptr(), wo.data_ptr(), wgu.data_ptr(), wdown.data_ptr()
            # frozen attention biases (Qwen2: q|k|v; attention_bias: o as well), in the model dtype, one [d + 2 dkv] vector like wqkv's rows
            if getattr(cfg, "qkv_bias", False):
                ly.bqkv = put(torch.cat([sd[p + f"self_attn.{nm}.bias"] for nm in LORA_TARGETS[:3]], 0), (i, "bqkv")).data_ptr()
            if getattr(cfg, "o_bias", False):
                ly.bo = put_sd(p + "self_attn.o_proj.bias").data_ptr()
            # frozen per-head q/k RMSNorm weights [hd] (Qwen3), in the model dtype like every norm weight (fp32 mode keeps them fp32)
            if getattr(cfg, "qk_norm", False):
                ly.q_norm_w = put_sd(p + "self_attn.q_norm.weight").data_ptr()
                ly.k_norm_w = put_sd(p + "self_attn.k_norm.weight").data_ptr()
            if training:
                self.attn_wt[i] = (put(wqkv.t()), put(wo.t()))
                ly.wqkv_t, ly.wo_t = (t.data_ptr() for t in self.attn_wt[i])
                self.mlp_wt[i] = (put(wgu.t()), put(wdown.t()))
                ly.wgu_t, ly.wdown_t = (t.data_ptr() for t in self.mlp_wt[i])
            if self.fp8 or self.decode_fp8:
                ly.wqkv8, ly.sqkv8, ly.eqkv8 = images(wqkv, key=(i, "qkv"))
                ly.wo8, ly.so8, ly.eo8 = images(wo, key=(i, "o"))
                ly.wgu8, ly.sgu8, ly.egu8 = images(wgu, key=(i, "gu"))
                ly.wdown8, ly.sdown8, ly.edown8 = images(wdown, key=(i, "down"))
            if self.decode_fp4:
                img4 = self._fp4_images(ly, wqkv, wo, wgu, wdown)
                for nm4 in ("qkv", "o", "gu", "down"):
                    self.img4[i, nm4] = img4[nm4]
            if self.use_lora:
                es = self.img_A.element_size()
                for k, nm in enumerate(LORA_MLP_MODULES):
                    if nm not in self.targets:
                        continue
                    lm, im = ly.lora_mlp[k], self.mlp_img[nm]
                    lm.A_pad, lm.B_pad, lm.BT_pad = im["A"][i].data_ptr(), im["B"][i].data_ptr(), im["BT"][i].data_ptr()
                    lm.AT_pad, lm.ld_at = im["AT"][i].data_ptr() + im["at_col"] * es, im["ld_at"]
                    a, b = self._slices(i, nm)
                    lm.gA = self.lora_g[a[0]:a[1]].data_ptr()
                    lm.gB = self.lora_g[b[0]:b[1]].data_ptr()
                for j in range(4):
                    if LORA_TARGETS[j] not in self.targets:
                        continue
                    lm = ly.lora[j]
                    lm.A_pad = self.img_A[i, j].data_ptr()
                    lm.B_pad = self.img_B[i][j].data_ptr()
                    lm.BT_pad = self.img_BT[i][j].data_ptr()
                    if j < 3:
                        lm.AT_pad, lm.ld_at = self.img_ATqkv[i].data_ptr() + j * L.LORA_PAD * es, 3 * L.LORA_PAD
                    else:
                        lm.AT_pad, lm.ld_at = self.img_ATo[i].data_ptr(), L.LORA_PAD
                    a, b = self._slices(i, j)
                    lm.gA = self.lora_g[a[0]:a[1]].data_ptr()
                    lm.gB = self.lora_g[b[0]:b[1]].data_ptr()
        m.layer = C.cast(self.layers, C.POINTER(L.LlamaLayer))
        self.desc = m
        self.ws = Workspace(device)            # training: holds the saved activations between fwd_loss() and bwd()
        self.ws_infer = Workspace(device)      # prefill / decode_step scratch: an eval forward or generate() between a training
        self._last = None                      #   forward and its backward must not touch the saved activations
        self.acc = torch.zeros(2, dtype=torch.float32, device=device)     # [loss_sum, count]
        self.loss_opts = None       # avllm_loss_opts of the last fwd_loss() with label smoothing or z-loss on, else None
        self.loss_terms = None      # [sum nll, sum (lse - mean logit), sum lse^2]: owned from the first fwd_loss() with label smoothing or z-loss on
        if self.use_lora:
            self.pack_lora()

    def _fp4_images(self, ly, wqkv, wo, wgu, wdown):
        """MXFP4 codes + exponents of one layer's four frozen matrices into its descriptor (tensors parked in self.keep); returns them by
        matrix name."""
        out = {}
        for nm, wt in (("qkv", wqkv), ("o", wo), ("gu", wgu), ("down", wdown)):
            q4, e4 = out[nm] = ops.mx4_quantize(wt)
            self.keep += [q4, e4]
            setattr(ly, "w" + nm + "4", q4.data_ptr())
            setattr(ly, "e" + nm + "4", e4.data_ptr())
        return out

    # flat-buffer offsets of module j (its name, or 0..6 = q,k,v,o,gate,up,down) in layer i: (A range, B range).  A layer holds the selected
    # modules only, in canonical order
    def _slices(self, i, j):
        nm = j if isinstance(j, str) else LORA_MODULES[j]
        if nm not in self.targets:
            raise KeyError(f"{nm} carries no LoRA adapter in this engine (lora_target_modules = {', '.join(self.targets)})")
        base = i * self.per_layer
        (a0, a1), (b0, b1) = self._layout[nm]
        return (base + a0, base + a1), (base + b0, base + b1)

    def lora_views(self, buf=None):
        """dict key -> fp32 view into the flat buffer, keys `layers.{i}.{module}.lora_A|B` (oracle naming)."""
        buf = self.lora_p if buf is None else buf
        out = {}
        for i in range(self.cfg.layers):
            for nm in self.targets:
                a, b = self._slices(i, nm)
                out[f"layers.{i}.{nm}.lora_A"] = buf[a[0]:a[1]].view(self.mod_shapes[nm][0])
                out[f"layers.{i}.{nm}.lora_B"] = buf[b[0]:b[1]].view(self.mod_shapes[nm][1])
        return out

    def _refuse_merged(self, what):
        if self.merged:
            raise RuntimeError(f"{what} needs the separate adapters, which merge_lora() folded into the LLM weights for good")

    def load_lora(self, lora_sd):
        self._refuse_merged("load_lora()")
        v = self.lora_views()
        for k, t in lora_sd.items():
            if k not in v:      # never dropped in silence: a tensor of a module this model does not adapt is a mismatch of the two
                raise KeyError(f"load_lora(): {k} is a LoRA tensor of a module this model does not adapt "
                               f"(lora_target_modules = {', '.join(self.targets)})")
            v[k].copy_(t.to(device=self.device, dtype=torch.float32))

    def pack_lora(self):
        """Refresh the padded operand images from the fp32 masters (after every optimizer step): one launch for all adapters,
        driven by a device-side table of (master, image) pointers built on first use."""
        self._refuse_merged("pack_lora()")
        lib = L.load()
        if getattr(self, "_pack_table", None) is None:
            rows, rows_f = [], []                       # adapters that read d-wide inputs; down_proj's, which read ffn-wide ones
            for i in range(self.cfg.layers):
                for nm in self.targets:
                    j = LORA_MODULES.index(nm)
                    a, b = self._slices(i, nm)
                    lm = self.layers[i].lora[j] if j < 4 else self.layers[i].lora_mlp[j - 4]
                    (rows_f if nm == "down_proj" else rows).append(
                        [self.lora_p[a[0]:a[1]].data_ptr(), self.lora_p[b[0]:b[1]].data_ptr(), lm.A_pad, lm.AT_pad, lm.B_pad, lm.BT_pad, lm.ld_at,
                         self.mod_shapes[nm][1][0]])
            self._pack_table = torch.tensor(rows, dtype=torch.int64, device=self.device) if rows else None
            self._pack_table_f = torch.tensor(rows_f, dtype=torch.int64, device=self.device) if rows_f else None
        # avllm_lora_pack_batch takes one input width per call
        for table, din in ((self._pack_table, self.cfg.hidden), (self._pack_table_f, self.cfg.ffn)):
            if table is not None:
                L.check(lib.avllm_lora_pack_batch(L.ptr(table), table.shape[0], self.r, din, self.desc.dtype, L.stream_ptr()))

    # ------------------------------------------------------------------ training
    def fwd_loss(self, x, labels, want_logits=False, dropout=0.0, seed=0, seed_dev=None, label_smoothing=0.0, z_loss=0.0):
        """x [B,S,d] (engine dtype), labels int64 [B,S] (-100 applied).  Leaves loss_sum,count in self.acc.
        `dropout`/`seed`: lora_dropout probability and the step's mask seed (kept in the descriptor for bwd()); `seed_dev`: device
        pointer (int) of a uint32 added to `seed` at run time -- the step state of a graph-replayable step.
        `label_smoothing`/`z_loss`: the objective of avllm_ce_smooth_fwd, kept in self.loss_opts (avllm_loss_opts) so that bwd() hands the
        backward the forward's values; with either on, loss_sum is the sum of the composite terms and self.loss_terms holds the raw sums
        [nll, lse - mean logit, lse^2], zeroed beside self.acc.  With both 0 the entries without options are called, as ever: the plain cross
        entropy, nothing allocated, self.loss_opts None."""
        self._refuse_merged("fwd_loss()")
        lib = L.load()
        eps, zeta = ops.check_loss_options(label_smoothing, z_loss)
        if eps or zeta:
            if self.loss_terms is None:
                self.loss_terms = torch.zeros(3, dtype=torch.float32, device=self.device)
            self.loss_terms.zero_()
            self.loss_opts = L.LossOpts(eps, zeta, self.loss_terms.data_ptr())
        else:
            self.loss_opts = None
        self.desc.lora_dropout = float(dropout) if self.use_lora else 0.0
        self.desc.dropout_seed = int(seed) & 0xFFFFFFFF
        self.desc.dropout_seed_dev = seed_dev
        B, S, _ = x.shape
        x = x.contiguous()
        labels = labels.contiguous()
        ws = self.ws.get(lib.avllm_llama_train_workspace_bytes(C.byref(self.desc), B, S))
        logits = torch.empty(B, S, self.cfg.vocab, device=self.device, dtype=self.dtype) if want_logits else None
        self.acc.zero_()
        if self.loss_opts is not None:
            L.check(lib.avllm_llama_lora_fwd_loss_opts(C.byref(self.desc), L.ptr(x), L.ptr(labels), B, S, L.ptr(logits), L.ptr(self.acc),
                                                       L.ptr(self.acc) + 4, C.byref(self.loss_opts), L.ptr(ws), ws.numel(), L.stream_ptr()))
        else:
            L.check(lib.avllm_llama_lora_fwd_loss(C.byref(self.desc), L.ptr(x), L.ptr(labels), B, S, L.ptr(logits), L.ptr(self.acc),
                                                  L.ptr(self.acc) + 4, L.ptr(ws), ws.numel(), L.stream_ptr()))
        self._last = (B, S, labels, ws.data_ptr(), ws.numel())
        self.gen = getattr(self, "gen", 0) + 1          # identifies whose activations the workspace holds (checked by _LoraLoss.backward)
        return logits

    def bwd(self, grad_scale=1.0, count=None, after_layer=None, layer_hi=None, layer_lo=0, dx_embeds=None):
        """Accumulates LoRA grads into self.lora_g (zero it first).  `count` = device float tensor holding the
        (possibly all-reduced) number of scored tokens; defaults to this rank's.  layer_hi/layer_lo: run only that piece of the
        backward pass (decoder layers layer_hi .. layer_lo; pieces in descending order, avllm_llama_lora_bwd_layers).
        dx_embeds: [B,S,d] tensor of the engine dtype that receives d loss / d inputs_embeds when the piece reaches layer 0
        (avllm_llama_lora_bwd_layers_dx; the connectors' gradient starts there)."""
        self._refuse_merged("bwd()")
        lib = L.load()
        if self._last is None:
            raise RuntimeError("LlamaEngine.bwd() without a preceding fwd_loss()")
        B, S, labels, ws_ptr, ws_len = self._last
        ws = self.ws.buf
        if ws is None or ws.data_ptr() != ws_ptr or ws.numel() != ws_len:
            raise RuntimeError("LlamaEngine.bwd(): the training workspace changed since fwd_loss() (the saved activations are gone)")
        cnt = self.acc[1:2] if count is None else count
        cb = L.LAYER_CB(lambda l, u: after_layer(l)) if after_layer is not None else L.LAYER_CB(0)
        hi = self.cfg.layers - 1 if layer_hi is None else layer_hi
        if dx_embeds is not None and (dx_embeds.dtype != self.dtype or dx_embeds.numel() != B * S * self.cfg.hidden or not dx_embeds.is_contiguous()):
            raise ValueError(f"LlamaEngine.bwd(): dx_embeds must be a contiguous [{B},{S},{self.cfg.hidden}] {self.dtype} tensor")
        if self.loss_opts is not None:      # the objective of the forward whose activations the workspace holds
            L.check(lib.avllm_llama_lora_bwd_layers_dx_opts(C.byref(self.desc), L.ptr(labels), B, S, L.ptr(cnt), grad_scale, L.ptr(ws), ws.numel(),
                                                            hi, layer_lo, cb, None, L.ptr(dx_embeds), C.byref(self.loss_opts), L.stream_ptr()))
            return
        if dx_embeds is not None:
            if dx_embeds.dtype != self.dtype or dx_embeds.numel() != B * S * self.cfg.hidden or not dx_embeds.is_contiguous():
                raise ValueError(f"LlamaEngine.bwd(): dx_embeds must be a contiguous [{B},{S},{self.cfg.hidden}] {self.dtype} tensor")
            L.check(lib.avllm_llama_lora_bwd_layers_dx(C.byref(self.desc), L.ptr(labels), B, S, L.ptr(cnt), grad_scale, L.ptr(ws), ws.numel(),
                                                       hi, layer_lo, cb, None, L.ptr(dx_embeds), L.stream_ptr()))
            return
        L.check(lib.avllm_llama_lora_bwd_layers(C.byref(self.desc), L.ptr(labels), B, S, L.ptr(cnt), grad_scale, L.ptr(ws), ws.numel(),
                                                hi, layer_lo, cb, None, L.stream_ptr()))

    # ------------------------------------------------------------------ inference
    def adapters_disabled(self):
        """Context manager: the LLM without its LoRA adapters, as scripts/clip_whisper/decode.py of the reference runs it (it rebuilds the
        model with use_lora=False and loads the connector weights only, decode.py:186-197,236-260)."""
        self._refuse_merged("adapters_disabled()")
        eng = self

        mods = lambda ly: [ly.lora[j] for j in range(4)] + [ly.lora_mlp[k] for k in range(3)]      # all seven modules

        class _Ctx:
            def __enter__(self_):
                self_.saved = [[(lm.A_pad, lm.B_pad) for lm in mods(ly)] for ly in eng.layers]
                for ly in eng.layers:
                    for lm in mods(ly):
                        lm.A_pad = None
                        lm.B_pad = None

            def __exit__(self_, *a):
                for ly, sv in zip(eng.layers, self_.saved):
                    for lm, (pa, pb) in zip(mods(ly), sv):
                        lm.A_pad, lm.B_pad = pa, pb
        return _Ctx()

    def merge_lora(self):
        """Fold the adapters into the LLM weights for decoding, for good: W' = W + scale * B.A on q, k, v (row slices of wqkv), o, gate, up
        (the row halves of wgu) and down -- the adapted ones among them -- from the fp32 masters (avllm_lora_merge), every fp8 / fp4 image of
        the matrices written to rebuilt in place by the quantisers that made it, and the adapter pointers cleared, so that prefill and the
        token step take the adapter-free kernels (the fused token step, which an adapter on gate, up or down keeps a model from).  lora_p
        stays (state_dict() still returns the adapters); the transposed training copies of wqkv and wo, and with an MLP adapter those of wgu
        and wdown, are stale afterwards and freed, and everything that would need the separate adapters back raises."""
        if not self.use_lora:
            raise ValueError("merge_lora(): this engine has no LoRA adapters (use_lora=False)")
        self._refuse_merged("a second merge_lora()")
        v = self.lora_views()
        rows = self._qkv_rows()
        f = self.cfg.ffn
        for i in range(self.cfg.layers):
            ly = self.layers[i]

            def own(key, field):
                # wqkv and wgu were concatenated here, but wo and wdown may be the caller's own tensors (a state dict already on the device in
                # the engine dtype is taken as it is): the merge writes into a copy the engine owns
                old = self.llm_w[key]
                new = self.llm_w[key] = old.clone()
                self.keep = [new if t is old else t for t in self.keep]
                setattr(ly, field, new.data_ptr())
                return new

            wqkv, wgu = self.llm_w[i, "qkv"], self.llm_w[i, "gu"]
            wo = own(f"model.layers.{i}.self_attn.o_proj.weight", "wo")
            wdown = own(f"model.layers.{i}.mlp.down_proj.weight", "wdown") if "down_proj" in self.targets else None
            where = {"q_proj": lambda: wqkv[rows[0][0]:rows[0][1]], "k_proj": lambda: wqkv[rows[1][0]:rows[1][1]],
                     "v_proj": lambda: wqkv[rows[2][0]:rows[2][1]], "o_proj": lambda: wo,
                     "gate_proj": lambda: wgu[:f], "up_proj": lambda: wgu[f:], "down_proj": lambda: wdown}
            for nm in self.targets:
                j = LORA_MODULES.index(nm)
                ops.lora_merge_(where[nm](), v[f"layers.{i}.{nm}.lora_A"], v[f"layers.{i}.{nm}.lora_B"], self.lcfg.scale)
                lm = ly.lora[j] if j < 4 else ly.lora_mlp[j - 4]
                lm.A_pad = None
                lm.B_pad = None
            touched = [("qkv", wqkv), ("o", wo)]
            if "gate_proj" in self.targets or "up_proj" in self.targets:
                touched.append(("gu", wgu))
            if wdown is not None:
                touched.append(("down", wdown))
            for nm, W in touched:
                if (i, nm) in self.img8:
                    q, s, e = self.img8[i, nm]
                    if s is not None:
                        ops.mx_quantize(W, 1, q=q, s=s)
                    if e is not None:
                        ops.mx_quantize(W, 2, q=q, s=e)
                if (i, nm) in self.img4:
                    ops.mx4_quantize(W, out=self.img4[i, nm])
            if i in self.attn_wt:
                stale = {t.data_ptr() for t in self.attn_wt.pop(i)}
                self.keep = [t for t in self.keep if t.data_ptr() not in stale]
                ly.wqkv_t = ly.wo_t = None
            if i in self.mlp_wt and self.mlp_targets:      # the transposed copies of wgu and wdown are stale as well
                stale = {t.data_ptr() for t in self.mlp_wt.pop(i)}
                self.keep = [t for t in self.keep if t.data_ptr() not in stale]
                ly.wgu_t = ly.wdown_t = None
        self.merged = True

    def merged_llm_state_dict(self):
        """The whole LLM after merge_lora() under its HuggingFace names: clones in the engine dtype, wqkv split back into q_proj, k_proj and
        v_proj, the fused gate/up matrix into its halves.  A use_lora=False model built from it computes what this engine computes."""
        if not self.merged:
            raise RuntimeError("merged_llm_state_dict() comes after merge_lora()")
        out, f = {}, self.cfg.ffn
        for name, t in self.llm_w.items():
            if isinstance(name, str):
                out[name] = t.clone()
                continue
            i, what = name
            p = f"model.layers.{i}."
            if what == "gu":
                out[p + "mlp.gate_proj.weight"], out[p + "mlp.up_proj.weight"] = t[:f].clone(), t[f:].clone()
            else:                                  # "qkv" (weight rows) or "bqkv" (the bias vector laid out like them)
                kind = "weight" if what == "qkv" else "bias"
                for nm, (lo, hi) in zip(LORA_TARGETS[:3], self._qkv_rows()):
                    out[p + f"self_attn.{nm}.{kind}"] = t[lo:hi].clone()
        return out

    def _qkv_rows(self):
        """Row ranges of q, k and v in the fused wqkv."""
        d, dkv = self.cfg.hidden, self.dkv
        return (0, d), (d, d + dkv), (d + dkv, d + 2 * dkv)

    def frozen_weight_bytes(self):
        """Bytes of frozen weights ONE decode token step streams from HBM: every projection of every layer + lm_head (the embedding
        table contributes B rows, the norms 2 vectors per layer: both negligible and left out)."""
        d, f = self.cfg.hidden, self.cfg.ffn
        per_layer = (d + 2 * self.dkv) * d + d * d + 2 * f * d + d * f
        return (self.cfg.layers * per_layer + self.cfg.vocab * d) * (4 if self.dtype == torch.float32 else 2)

    def decode_is_fused(self, B):
        """True when a token step of B sequences takes the fused bf16 path (tests and benchmarks assert which path they measured)."""
        return bool(L.load().avllm_llama_decode_is_fused(C.byref(self.desc), B))

    def decode_streams_fp8(self, B):
        """True when a token step of B sequences streams the fp8 weight images (decode_fp8 and the fused path: B <= 16)."""
        return bool(L.load().avllm_llama_decode_streams_fp8(C.byref(self.desc), B))

    def decode_streams_fp4(self, B):
        """True when a token step of B sequences streams the MXFP4 weight images (decode_fp4 and the fused path: B <= 16)."""
        return bool(L.load().avllm_llama_decode_streams_fp4(C.byref(self.desc), B))

    def streamed_weight_bytes(self, B):
        """Bytes of frozen weights a token step of B sequences actually reads: frozen_weight_bytes() on the bf16 matrices, or one byte per
        element plus one exponent byte per 32 elements when the step streams fp8, or half a byte per projection element, one byte per
        lm_head element (e4m3) and one exponent byte per 32 elements of both when it streams fp4."""
        if self.decode_streams_fp4(B):
            proj = (self.frozen_weight_bytes() // 2) - self.cfg.vocab * self.cfg.hidden      # elements of the layers' projections
            head = self.cfg.vocab * self.cfg.hidden
            return proj // 2 + proj // 32 + head + head // 32
        if not self.decode_streams_fp8(B):
            return self.frozen_weight_bytes()
        n = self.frozen_weight_bytes() // 2
        return n + n // 32

    def decode_caches_fp8(self, B):
        """True when a token step of B sequences runs on the fp8 cache image (kv_fp8 and the fused path: B <= 16, head dim 64 or 128)."""
        return bool(L.load().avllm_llama_decode_caches_fp8(C.byref(self.desc), B))

    def kv_cache_bytes(self, B, Tmax, fp8=None):
        """Bytes of K plus V for B sequences of Tmax positions, in the form alloc_cache(B, Tmax, fp8=fp8) hands out."""
        with self._cache_form(self.decode_caches_fp8(B) if fp8 is None else fp8):
            return 2 * L.load().avllm_llama_kv_cache_bytes(C.byref(self.desc), B, Tmax)

    def alloc_cache(self, B, Tmax, rows=None, fp8=None):
        """(K, V) caches of B sequences and Tmax positions.  The form is decided here: fp8 images (ops.kv8_alloc: uint8 [layers, B, Tmax,
        dkv + dkv/32]) when the engine has kv_fp8 and the token steps that will read the cache -- of `rows` sequences (default B; beam search
        prefills B and steps B * num_beams) -- take the fused path, else [layers, B, Tmax, dkv] in the engine dtype.  fp8=False: the latter
        whatever the engine's option (an eval forward keeps its bf16 cache)."""
        if fp8 is None:
            fp8 = self.decode_caches_fp8(B if rows is None else rows)
        if fp8:
            if not self.kv_fp8:
                raise ValueError("alloc_cache(fp8=True) on an engine built without kv_fp8")
            return tuple(ops.kv8_alloc(self.cfg.layers, B, Tmax, dkv=self.dkv, device=self.device) for _ in range(2))
        shape = (self.cfg.layers, B, Tmax, self.dkv)
        return torch.empty(shape, dtype=self.dtype, device=self.device), torch.empty(shape, dtype=self.dtype, device=self.device)

    def decode_shares_prefix(self, R):
        """True when a token step of R rows can read a prefix stored once per item (decode_step_shared): exactly where decode_is_fused(R)."""
        return bool(L.load().avllm_llama_decode_shares_prefix(C.byref(self.desc), R))

    def alloc_suffix_cache(self, R, N):
        """(K, V) suffix caches of a shared-prefix decode: R rows of N generated positions, in the form alloc_cache(..., rows=R) gives the
        prefix cache they go with."""
        return self.alloc_cache(R, N)

    def _cache_form(self, fp8):
        """Context manager: the descriptor's kv_fp8 says the form of the cache of the call inside, then is the engine's option again."""
        eng = self

        class _Ctx:
            def __enter__(self_):
                eng.desc.kv_fp8 = int(bool(fp8))

            def __exit__(self_, *a):
                eng.desc.kv_fp8 = int(eng.kv_fp8)
        return _Ctx()

    def _check_caches(self, kc, vc):
        """The form of a cache pair: True for fp8 images (uint8, checked here: the library sees only pointers), False for the engine dtype."""
        if kc.dtype != torch.uint8 and vc.dtype != torch.uint8:
            return False
        if not self.kv_fp8:
            raise ValueError("an fp8 KV cache needs an engine built with kv_fp8")
        if kc.shape != vc.shape or kc.dtype != vc.dtype or kc.dim() != 4 or kc.shape[3] != self.dkv + self.dkv // 32 or not (
                kc.is_contiguous() and vc.is_contiguous()):
            raise ValueError(f"fp8 KV caches must be a pair from alloc_cache(), got {tuple(kc.shape)} {kc.dtype} and {tuple(vc.shape)} {vc.dtype}")
        return True

    def prefill(self, x, kc, vc, all_logits=False):
        lib = L.load()
        B, S, _ = x.shape
        x = x.contiguous()
        Tmax = kc.shape[2]
        ws = self.ws_infer.get(lib.avllm_llama_infer_workspace_bytes(C.byref(self.desc), B, S))
        last = torch.empty(B, self.cfg.vocab, device=self.device, dtype=torch.float32)
        full = torch.empty(B, S, self.cfg.vocab, device=self.device, dtype=self.dtype) if all_logits else None
        with self._cache_form(self._check_caches(kc, vc)):
            L.check(lib.avllm_llama_prefill(C.byref(self.desc), L.ptr(x), B, S, L.ptr(kc), L.ptr(vc), Tmax, L.ptr(last), L.ptr(full),
                                            L.ptr(ws), ws.numel(), L.stream_ptr()))
        return last, full

    def decode_step(self, ids, pos, kc, vc, pos_dev=None, logits=None):
        """One token per sequence at position `pos` (+ the int32 in device memory `pos_dev`: a captured step replays for every token).
        `logits`: optional preallocated [B, vocab] float32 output."""
        lib = L.load()
        B = ids.shape[0]
        ws = self.ws_infer.get(lib.avllm_llama_infer_workspace_bytes(C.byref(self.desc), B, 1))
        if logits is None:
            logits = torch.empty(B, self.cfg.vocab, device=self.device, dtype=torch.float32)
        with self._cache_form(self._check_caches(kc, vc)):
            L.check(lib.avllm_llama_decode_step_at(C.byref(self.desc), L.ptr(ids.contiguous()), B, pos, L.ptr(pos_dev), L.ptr(kc), L.ptr(vc),
                                                   kc.shape[2], L.ptr(logits), L.ptr(ws), ws.numel(), L.stream_ptr()))
        return logits

    def decode_step_shared(self, ids, pos, k_prefix, v_prefix, k_suffix, v_suffix, group, pos_dev=None, logits=None):
        """One token per row of R = B * group rows whose `group` rows per item share the item's prefix: k_prefix, v_prefix [layers, B, S, dkv]
        are the caches prefill() wrote (exactly S positions; read only), k_suffix, v_suffix [layers, R, N, dkv] (alloc_suffix_cache) hold each
        row's generated positions.  The token runs at position S + pos (+ *pos_dev) and its K/V go to suffix row pos.  Needs
        decode_shares_prefix(R); only the attention launch differs from decode_step()."""
        lib = L.load()
        R = ids.shape[0]
        fp8 = self._check_caches(k_suffix, v_suffix)
        if self._check_caches(k_prefix, v_prefix) != fp8 or k_prefix.shape != v_prefix.shape or k_suffix.shape != v_suffix.shape:
            raise ValueError("decode_step_shared: prefix and suffix caches must be K/V pairs of one form (alloc_cache(B, S, rows=R), alloc_suffix_cache(R, N))")
        if group < 1 or k_prefix.shape[1] * group != R or k_suffix.shape[1] != R:
            raise ValueError(f"decode_step_shared: {R} rows need a prefix cache of {R} / group rows and a suffix cache of {R} rows, got group = {group}, "
                             f"{k_prefix.shape[1]} and {k_suffix.shape[1]}")
        ws = self.ws_infer.get(lib.avllm_llama_decode_shared_workspace_bytes(C.byref(self.desc), R))
        if logits is None:
            logits = torch.empty(R, self.cfg.vocab, device=self.device, dtype=torch.float32)
        with self._cache_form(fp8):
            L.check(lib.avllm_llama_decode_step_shared(C.byref(self.desc), L.ptr(ids.contiguous()), R, group, pos, L.ptr(pos_dev), L.ptr(k_prefix),
                                                       L.ptr(v_prefix), k_prefix.shape[2], L.ptr(k_suffix), L.ptr(v_suffix), k_suffix.shape[2],
                                                       L.ptr(logits), L.ptr(ws), ws.numel(), L.stream_ptr()))
        return logits
