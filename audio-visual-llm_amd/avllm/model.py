"""ClipWhisperModel -- host-side mirror of the reference class of the same name
(src/clip_whisper/models/clip_whisper_model.py:24-1451): same constructor keywords, attributes, methods,
argument meaning and error behaviour; every tensor op runs in libavllm.so (HIP, gfx950).

Differences that are deliberate and documented:
  * precision: `use_fp16=True` selects the MI355X reduced-precision mode (bf16 storage / fp32 accumulate);
    `use_fp16=False` is strict fp32 (fp32 MFMA).  `precision="bf16"|"fp32"` overrides.
  * weights come from local HF checkpoints (safetensors) when the given paths exist, from `_provided_*`
    modules' state_dict()s, from `weights=`, or -- only with `synthetic_weights=True` -- from a seeded synthetic
    initialisation of the named architecture (a path that is none of these raises FileNotFoundError).
  * freeze_encoders=False / use_4bit=True are refused (out of scope).
  * train_connectors=True (default False) trains the two modality connectors with the encoders frozen: the reference's freeze_encoders=False
    gradient (clip_whisper_model.py:1096-1106,1136-1146) restricted to the four connector tensors, which does not depend on whether the
    encoders receive one too.  connector_type "simple", precision fp32 | bf16, use_lora=True.
"""
from __future__ import annotations

import logging
import math
import numbers
import os
import types
from typing import NamedTuple, Optional

import torch

from . import lib as L
from . import ops
from .arch import ModelCfg, resolve_arch
from .connector import ModalityConnector, create_modality_connector
from .engine import ClipEngine, LlamaEngine, WhisperEngine
from .tokenizer import load_tokenizer, phrase_token_ids


def hotword_sequence_bias(tokenizer, hotwords, hotword_bias, sequence_bias=None):
    """generate(hotwords=, hotword_bias=) as a sequence_bias dict: each hotword is tokenised with and without a leading space (no special
    tokens), and every prefix t[:1] ... t[:L] of each distinct tokenisation gets hotword_bias, so the whole path of the word is boosted,
    not only its last token.  Prefixes shared by several hotwords are merged into one entry.  The user's own sequence_bias entries come
    first; a hotword prefix equal to one of their keys is a ValueError (which bias is meant cannot be told).
    HF's SequenceBiasLogitsProcessor considers a sequence of L tokens only once L tokens have been generated (L <= n, not L - 1 <= n), so
    token k > 1 of a hotword is not boosted while fewer than k tokens exist: a hotword that starts the utterance gets its first token
    boosted and the rest only from the point where the history is as long as the prefix."""
    if isinstance(hotwords, str) or not isinstance(hotwords, (list, tuple)) or any(not isinstance(w, str) or not w.strip() for w in hotwords):
        raise ValueError(f"hotwords must be a list of non-empty strings, got {hotwords!r}")
    if isinstance(hotword_bias, bool) or not isinstance(hotword_bias, numbers.Real) or not math.isfinite(hotword_bias):
        raise ValueError(f"hotword_bias must be a finite float, got {hotword_bias!r}")
    out = dict(ops._normalise_logits_bias(sequence_bias, None, None, None, None, None)[0] or {})
    user = set(out)
    for w in hotwords:
        for ids in phrase_token_ids(tokenizer, w):
            for k in range(1, len(ids) + 1):
                if ids[:k] in user:
                    raise ValueError(f"hotword {w!r}: its token prefix {ids[:k]} is also a sequence_bias key")
                out[ids[:k]] = float(hotword_bias)
    return out


class GenerateOutput(NamedTuple):
    """generate(return_token_scores=True).  sequences: int64 [rows, L] new tokens; sequences_scores: float32 [rows], beam search only
    (else None); token_scores: float32 [rows, L], the log-probability of every returned token (HF's compute_transition_scores), 0.0
    after a row's EOS or beyond a hypothesis' length; token_entropy: float32 [rows, L], the entropy in nats of the distribution each
    token was chosen from, masked the same way."""
    sequences: torch.Tensor
    sequences_scores: Optional[torch.Tensor]
    token_scores: torch.Tensor
    token_entropy: torch.Tensor


class _LoraLoss(torch.autograd.Function):
    """Makes `out["loss"].backward()` (trainer/clip_whisper_trainer.py:454) drive avllm_llama_lora_bwd; with train_connectors=True the four
    connector parameters are inputs too and receive their gradients from the same backward pass."""

    @staticmethod
    def forward(ctx, lora_param, model, loss_value, *connector_params):
        ctx.model = model
        ctx.gen = model.llm_engine.gen
        return loss_value.clone()

    @staticmethod
    def backward(ctx, grad_out):
        m = ctx.model
        eng = m.llm_engine
        if eng.gen != ctx.gen:
            raise RuntimeError("loss.backward(): another training forward ran since this loss was computed; its activations were overwritten")
        eng.lora_g.zero_()
        if not m.train_connectors:
            eng.bwd(grad_scale=float(grad_out))
            return eng.lora_g.clone(), None, None
        eng.bwd(grad_scale=float(grad_out), dx_embeds=m._dx_embeds_buffer())
        m.connector_backward()
        return (eng.lora_g.clone(), None, None) + tuple(g.clone() for g in m.connector_grad_views())


class ClipWhisperModel:
    def __init__(self, llm_path="meta-llama/Llama-2-7b-hf", whisper_model="openai/whisper-small",
                 clip_model="openai/clip-vit-base-patch16", device="cuda", use_fp16=False, use_4bit=False, use_lora=True,
                 lora_r=16, lora_alpha=32, lora_dropout=0.05, freeze_encoders=True, freeze_llm=False, modality="both",
                 max_seq_len=256, fusion_scale=0.5, connector_type="simple", _provided_tokenizer=None, _provided_llm=None,
                 _provided_whisper=None, _provided_clip=None, *, precision=None, config: ModelCfg | None = None,
                 weights: dict | None = None, seed: int = 0, synthetic_weights: bool = False, decode_weights: str = "bf16",
                 train_connectors: bool = False):
        if use_4bit:
            raise NotImplementedError("use_4bit (bitsandbytes nf4) is out of scope of the MI355X hot path (SURVEY.md §8)")
        if not freeze_encoders:
            raise NotImplementedError("freeze_encoders=False is not supported: the hot path trains LoRA only (SURVEY.md fact 4)")
        if modality not in ("audio", "video", "both"):
            raise ValueError(f"modality must be audio|video|both, got {modality}")
        L.load()                                   # fail loudly when the HIP library is missing
        self.device = device
        self.use_fp16, self.use_4bit, self.use_lora = use_fp16, use_4bit, use_lora
        if use_lora and "llama" not in str(llm_path).lower():
            # clip_whisper_model.py:966-970 picks target modules ["query","key","value","dense"] for such paths; no Llama/Mistral
            # module carries those names, so peft raises and the reference "continues without LoRA" (:1002-1005).  This build
            # attaches the q/k/v/o adapters to every Llama-architecture model instead.
            logging.warning("LLM path %r does not contain 'llama': the reference would train without LoRA here; "
                            "this build applies LoRA to q_proj/k_proj/v_proj/o_proj", llm_path)
        self.lora_r, self.lora_alpha, self.lora_dropout = lora_r, lora_alpha, lora_dropout
        self.freeze_encoders, self.freeze_llm = freeze_encoders, freeze_llm
        self.modality, self.max_seq_len, self.fusion_scale = modality, max_seq_len, fusion_scale
        self.connector_type = connector_type
        precision = precision or ("bf16" if use_fp16 else "fp32")
        if precision not in ("fp32", "bf16", "fp8"):
            raise ValueError(f"precision must be fp32|bf16|fp8, got {precision}")
        # "fp8" (BASELINE config 5): bf16 storage, with every frozen-weight projection of the encoders and of the LLM's training forward
        # on the block-scaled fp8 matrix pipe; attention, norms, LoRA terms, loss and the whole backward pass as in "bf16"
        self.fp8 = precision == "fp8"
        self.precision = precision
        # decode_weights="fp8": generate()'s token steps (greedy, sampling, beam search) stream the LLM's frozen projections as e4m3 codes with
        # one E8M0 exponent per 32 elements (weight-only; activations, KV cache and logits as in bf16).  Prefill and steps of more than 16
        # rows keep the bf16 weights.  A runtime choice: not saved with the model.
        # decode_weights="fp4": the same, with the four projections of every layer as OCP MXFP4 codes (e2m1, one E8M0 exponent per 32
        # elements) and lm_head as e4m3.  Far coarser than e4m3 (about 11.5 % relative L2 error on Gaussian weights); its effect on WER is
        # not measured.  Not use_4bit: that flag means bitsandbytes NF4 in the reference and stays refused.
        if decode_weights not in ("bf16", "fp8", "fp4"):
            raise ValueError(f"decode_weights must be bf16|fp8|fp4, got {decode_weights!r}")
        if decode_weights != "bf16" and precision == "fp32":
            raise ValueError(f"decode_weights='{decode_weights}' needs precision bf16 or fp8 (the {decode_weights} token step is a bf16-activation path)")
        self.decode_weights = decode_weights
        self.train_connectors = bool(train_connectors)
        if self.train_connectors:
            if connector_type != "simple":
                raise NotImplementedError(f"train_connectors=True supports connector_type='simple' only, got {connector_type!r}")
            if precision == "fp8":
                raise NotImplementedError("train_connectors=True supports precision fp32 | bf16, not fp8")
            if not use_lora:
                raise ValueError("train_connectors=True needs use_lora=True: the LoRA backward pass is the only LLM backward pass in the library")
        self.dtype = torch.float32 if precision == "fp32" else torch.bfloat16
        self.training = True
        self._drop_step = 0
        self._seed = int(seed or 0)

        cfg, W = resolve_arch(llm_path, whisper_model, clip_model, config, weights, seed, lora_r, lora_alpha, use_lora,
                              _provided_llm, _provided_whisper, _provided_clip, device, self.dtype, synthetic_weights)
        cfg.max_seq_len, cfg.fusion_scale = max_seq_len, fusion_scale
        self.cfg = cfg
        # explicit `weights=` / `config=` builds (tests, bench) are synthetic by construction: they carry no tokenizer either
        self.tokenizer = _provided_tokenizer or load_tokenizer(llm_path, cfg.llama.vocab, synthetic=synthetic_weights or weights is not None)
        if getattr(self.tokenizer, "pad_token_id", None) is None:
            self.tokenizer.pad_token_id = getattr(self.tokenizer, "eos_token_id", 2)      # pad = eos (:955-959)
        cfg.pad_token_id = self.tokenizer.pad_token_id
        self.whisper_processor = None
        self.clip_processor = None
        self.audio_dim, self.video_dim, self.llm_dim = cfg.whisper.d_model, cfg.clip.hidden, cfg.llama.hidden

        self.whisper_engine = WhisperEngine(W["whisper"], cfg.whisper, self.dtype, device, fp8=self.fp8) if modality in ("audio", "both") else None
        self.clip_engine = ClipEngine(W["clip"], cfg.clip, self.dtype, device, fp8=self.fp8) if modality in ("video", "both") else None
        self.llm_engine = LlamaEngine(W["llama"], cfg.llama, cfg.lora if use_lora else None, W.get("lora"), self.dtype, device,
                                      training=True, fp8=self.fp8, decode_fp8=decode_weights == "fp8", decode_fp4=decode_weights == "fp4")
        self._setup_projections(W)
        self.lora_param = None
        if use_lora:
            self.lora_param = torch.nn.Parameter(self.llm_engine.lora_p, requires_grad=not freeze_llm)
        self.eos_token_id = getattr(self.tokenizer, "eos_token_id", 2)

    # ------------------------------------------------------------------ plumbing mirrored from nn.Module
    def train(self, mode=True):
        self.training = mode
        return self

    def eval(self):
        return self.train(False)

    def to(self, *a, **k):
        return self

    def parameters(self):
        ps = [p for c in (self.audio_connector, self.video_connector) for p in c.parameters()]
        if self.lora_param is not None:
            ps.append(self.lora_param)
        return ps

    def named_parameters(self):
        out = [(f"audio_connector.{n}", p) for n, p in self.audio_connector.named_parameters()]
        out += [(f"video_connector.{n}", p) for n, p in self.video_connector.named_parameters()]
        if self.lora_param is not None:
            out.append(("llm.lora_flat", self.lora_param))
        return out

    def state_dict(self):
        """Trainable/connector tensors under the reference's key names (decode.py:237-238 matches by substring;
        LoRA uses the peft naming `llm.base_model.model.model.layers.N.self_attn.X.lora_A.default.weight`)."""
        sd = {f"audio_connector.{k}": v.detach().clone() for k, v in self.audio_connector.state_dict().items()}
        sd.update({f"video_connector.{k}": v.detach().clone() for k, v in self.video_connector.state_dict().items()})
        if self.use_lora:
            for k, v in self.llm_engine.lora_views().items():
                _, i, mod, ab = k.split(".")
                sd[f"llm.base_model.model.model.layers.{i}.self_attn.{mod}.{ab}.default.weight"] = v.detach().clone()
        return sd

    def load_state_dict(self, sd, strict=False):
        a = {k.split("audio_connector.")[1]: v for k, v in sd.items() if "audio_connector." in k}
        v_ = {k.split("video_connector.")[1]: v for k, v in sd.items() if "video_connector." in k}
        if a:
            self.audio_connector.load_state_dict(a)
        if v_:
            self.video_connector.load_state_dict(v_)
        lora = {}
        for k, t in sd.items():
            if ".lora_A." in k or ".lora_B." in k:
                parts = k.split(".")
                i = parts[parts.index("layers") + 1]
                mod = parts[parts.index("self_attn") + 1]
                ab = "lora_A" if ".lora_A." in k else "lora_B"
                lora[f"layers.{i}.{mod}.{ab}"] = t
        if lora and self.use_lora:
            self.llm_engine.load_lora(lora)
            self.llm_engine.pack_lora()
        return types.SimpleNamespace(missing_keys=[], unexpected_keys=[])

    def save_pretrained(self, output_dir):
        """Directory layout of clip_whisper_model.py:738-798 for the tensors this build owns."""
        os.makedirs(output_dir, exist_ok=True)
        # train_connectors=True: the parameters are views of one flat buffer and torch.save writes a view's whole storage, so they are cloned
        own = (lambda sd: {k: v.detach().clone() for k, v in sd.items()}) if self.train_connectors else (lambda sd: sd)
        torch.save(own(self.audio_connector.state_dict()), os.path.join(output_dir, "audio_connector.pt"))
        torch.save(own(self.video_connector.state_dict()), os.path.join(output_dir, "video_connector.pt"))
        import json
        cfg = dict(modality=self.modality, max_seq_len=self.max_seq_len, fusion_scale=self.fusion_scale, use_lora=self.use_lora,
                   lora_r=self.lora_r, lora_alpha=self.lora_alpha, connector_type=self.connector_type,
                   audio_dim=self.audio_dim, video_dim=self.video_dim, llm_dim=self.llm_dim)
        json.dump(cfg, open(os.path.join(output_dir, "config.json"), "w"), indent=2)
        torch.save(cfg, os.path.join(output_dir, "config.pt"))
        if self.use_lora:
            os.makedirs(os.path.join(output_dir, "llm"), exist_ok=True)
            torch.save({k: v for k, v in self.state_dict().items() if "lora_" in k}, os.path.join(output_dir, "llm", "adapter_model.pt"))

    @classmethod
    def from_pretrained(cls, model_dir, tokenizer=None, **kwargs):
        """clip_whisper_model.py:821-864.  The reference's own pair is not closed: its save_pretrained writes `config.pt` / `config.json` while its
        from_pretrained demands `model_config.json` (and `whisper/`, `clip/` directories that are only written with freeze_encoders=False), so it
        cannot reload what it saved.  This one reloads what save_pretrained above wrote -- connectors, adapters, the saved settings -- on top of
        base checkpoints named by the usual constructor keywords (`llm_path=`, `whisper_model=`, `clip_model=`, or `config=` + `synthetic_weights=`)."""
        import json
        if not os.path.exists(model_dir):
            raise ValueError(f"Model directory {model_dir} does not exist")
        cfg_path = os.path.join(model_dir, "config.json")
        if not os.path.exists(cfg_path):
            raise ValueError(f"Model config {cfg_path} does not exist")
        cfg = json.load(open(cfg_path))
        for k in ("modality", "max_seq_len", "fusion_scale", "use_lora", "lora_r", "lora_alpha", "connector_type"):
            if k in cfg:
                kwargs.setdefault(k, cfg[k])
        model = cls(_provided_tokenizer=tokenizer, **kwargs)
        model.audio_connector.load_state_dict(torch.load(os.path.join(model_dir, "audio_connector.pt"), map_location=model.device, weights_only=True))
        model.video_connector.load_state_dict(torch.load(os.path.join(model_dir, "video_connector.pt"), map_location=model.device, weights_only=True))
        adapters = os.path.join(model_dir, "llm", "adapter_model.pt")
        if model.use_lora and os.path.exists(adapters):
            model.load_state_dict(torch.load(adapters, map_location="cpu", weights_only=True))
        return model

    def _setup_projections(self, W=None):
        """clip_whisper_model.py:1159-1190: both connectors always exist."""
        # xavier init as in the reference, but drawn from a private generator state derived from `seed` (the global RNG is left alone):
        # two builds with the same seed are the same model, which the reference's unseeded nn.Linear init does not give
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(0x5EED + int(self._seed))
            kw = {"trainable": True} if self.train_connectors else {}
            self.audio_connector = create_modality_connector(self.connector_type, self.audio_dim, self.llm_dim, self.device, self.dtype, **kw)
            self.video_connector = create_modality_connector(self.connector_type, self.video_dim, self.llm_dim, self.device, self.dtype, **kw)
        if W is not None:
            if "audio_connector" in W:
                self.audio_connector.load_state_dict(W["audio_connector"])
            if "video_connector" in W:
                self.video_connector.load_state_dict(W["video_connector"])
        if self.train_connectors:
            self._flatten_connectors()

    def _flatten_connectors(self):
        """train_connectors=True: the four fp32 masters become views of ONE flat buffer `conn_p` in named_parameters() order (audio weight,
        audio bias, video weight, video bias) with the gradient buffer `conn_g` beside it, as the LoRA tensors live in lora_p / lora_g: the
        trainer's clip + AdamW and the data-parallel all-reduce each take them as one more flat buffer."""
        from .engine import Workspace
        ps = [p for c in (self.audio_connector, self.video_connector) for p in c.parameters()]
        n = sum(p.numel() for p in ps)
        self.conn_p = torch.empty(n, dtype=torch.float32, device=ps[0].device)
        self.conn_g = torch.zeros(n, dtype=torch.float32, device=ps[0].device)
        self.conn_slices, off = [], 0
        for p in ps:
            view = self.conn_p[off:off + p.numel()].view(p.shape)
            view.copy_(p.detach())
            p.data = view
            self.conn_slices.append((off, off + p.numel(), tuple(p.shape)))
            off += p.numel()
        self._conn_ws = {k: Workspace(self.device) for k in ("dx", "da", "dv")}
        self._conn_geo = None

    def connector_grad_views(self, buf=None):
        """The four gradient tensors [audio W, audio b, video W, video b] as views of conn_g (or of a buffer laid out like it)."""
        buf = self.conn_g if buf is None else buf
        return [buf[a:b].view(shape) for a, b, shape in self.conn_slices]

    def refresh_connectors(self):
        """After an update of the fp32 masters: rewrite the bf16 operand images (nothing to do in fp32 mode)."""
        self.audio_connector.refresh()
        self.video_connector.refresh()

    def _static(self, key, shape):
        n = 1
        for d in shape:
            n *= d
        n *= 4 if self.dtype == torch.float32 else 2
        return self._conn_ws[key].get(n)[:n].view(self.dtype).view(shape)

    def _dx_embeds_buffer(self):
        """Static [B,S,d] buffer for d loss / d inputs_embeds of the last training forward (LlamaEngine.bwd(dx_embeds=...))."""
        _, _, _, _, S, B = self._conn_geo
        return self._static("dx", (B, S, self.llm_dim))

    def connector_backward(self):
        """dx_embeds -> fuse / pool adjoint -> the two weight gradients and bias gradients, written into conn_g (overwritten, not
        accumulated).  The connectors' INPUT gradient is not formed: the encoders are frozen.  An input that was absent in the forward
        leaves its connector's gradient as zeros."""
        Ta, Tv, P, Lc, S, B = self._conn_geo
        D = self.llm_dim
        da = self._static("da", (B, Ta, D)) if Ta else None
        dv = self._static("dv", (B, Tv, D)) if Tv else None
        ops.fuse_pool_bwd(self._dx_embeds_buffer(), Ta, Tv, P, Lc, self.fusion_scale, da=da, dv=dv)
        gWa, gba, gWv, gbv = self.connector_grad_views()
        for dy, conn, gW, gb in ((da, self.audio_connector, gWa, gba), (dv, self.video_connector, gWv, gbv)):
            if dy is None:
                gW.zero_(); gb.zero_()
            else:
                ops.gemm_wgrad(dy.view(-1, D), conn.saved_input, dW=gW, db=gb)

    def _get_llm_dim(self):
        return self.cfg.llama.hidden

    # ------------------------------------------------------------------ encoders (+ connectors)
    def encode_audio(self, audio, attention_mask=None, rows=None):
        """clip_whisper_model.py:1067-1106.  `rows`: project only the first `rows` frames (identical result for the
        rows that survive encode()'s truncation, 3x fewer connector FLOPs at L=512)."""
        if audio is None:
            raise ValueError("Audio input cannot be None")
        nm = self.cfg.whisper.n_mels                               # the reference hard-codes 80 (:1074); lifted for whisper-large-v3 (128)
        if audio.dim() != 2 and (audio.dim() != 3 or audio.shape[1] != nm):
            raise ValueError(f"Audio input should have shape [batch_size, sequence_length] or [batch_size, {nm}, time_steps], but got {audio.shape}")
        if audio.dim() == 2:
            raise ValueError(f"raw-waveform audio is not supported: pass WhisperFeatureExtractor mel features [B,{nm},3000]")
        if self.whisper_engine is None:
            raise ValueError("audio encoder not loaded (modality=video)")
        h = self.whisper_engine.forward(audio)                       # [B,1500,d]
        return self.audio_connector(h if rows is None else h[:, :rows])

    def encode_video(self, video, attention_mask=None, rows=None):
        """clip_whisper_model.py:1108-1146: CLS of last_hidden_state per frame (no post_layernorm) -> connector."""
        if video.dim() != 5 or video.shape[2] != 3:
            raise ValueError(f"Video input should have shape [batch_size, frames, 3, height, width], but got {video.shape}")
        if self.clip_engine is None:
            raise ValueError("video encoder not loaded (modality=audio)")
        B, Fr = video.shape[:2]
        cls = self.clip_engine.forward(video.reshape(B * Fr, 3, video.shape[3], video.shape[4])).view(B, Fr, -1)
        return self.video_connector(cls if rows is None else cls[:, :rows])

    def _embed_prompt(self, prompt):
        if prompt is None:
            return None
        if isinstance(prompt, str):
            prompt = torch.tensor([self.tokenizer.encode(prompt)[:32]], dtype=torch.long)
        ids = prompt.to(self.device)[:, :32].contiguous()            # max_prompt_len = 32 (:469)
        return ops.embedding(self.llm_engine.embed, ids)

    def _features(self, audio, video):
        """(a_feat, v_feat, L) with the encode() modality rules (clip_whisper_model.py:407-445)."""
        a = v = None
        use_a = self.modality in ("audio", "both") and audio is not None
        use_v = self.modality in ("video", "both") and video is not None
        if use_a and use_v:
            if self.connector_type not in ("conv", "attention", "adaptive"):
                # per-token connectors (simple, deep = every unknown name): projecting only the rows that survive the truncation below is the
                # same function at a third of the connector FLOPs
                Ta, Tv = self.cfg.whisper.n_ctx, video.shape[1]
                Lc = min(self.max_seq_len, max(Ta, Tv))
                a = self.encode_audio(audio, rows=min(Ta, Lc))
                v = self.encode_video(video, rows=min(Tv, Lc))
                return a, v, Lc
            # sequence-mixing connectors (conv / attention / adaptive) see the whole sequence, and `adaptive` changes its length (T > 512 -> T / 4):
            # lengths are taken AFTER the connectors, as encode() does (:424-430)
            a, v = self.encode_audio(audio), self.encode_video(video)
            return a, v, min(self.max_seq_len, max(a.shape[1], v.shape[1]))
        if use_a:
            a = self.encode_audio(audio)
            return a, None, a.shape[1]
        if use_v:
            v = self.encode_video(video)
            return None, v, v.shape[1]
        raise ValueError("No valid inputs provided - both audio and video are None")

    def _llm_inputs(self, audio, video, prompt, S_out=None, keep=False):
        """keep (train_connectors=True, training forward): the connectors keep the rows they project and the fusion geometry is recorded,
        which is all connector_backward() needs -- no second encoder pass."""
        self.audio_connector.keep_input = self.video_connector.keep_input = bool(keep)
        try:
            a, v, Lc = self._features(audio, video)
        finally:
            self.audio_connector.keep_input = self.video_connector.keep_input = False
        pe = self._embed_prompt(prompt)
        P = pe.shape[1] if pe is not None else 0
        B = (a if a is not None else v).shape[0]
        S = P + Lc if S_out is None else S_out
        if keep:
            self._conn_geo = (a.shape[1] if a is not None else 0, v.shape[1] if v is not None else 0, P, Lc, S, B)
        return ops.fuse_pool(a, v, pe, Lc, S, self.fusion_scale, self.llm_dim, B)

    def encode(self, audio=None, video=None, prompt=None):
        """-> (inputs_embeds [B,P+L,D], attention_mask ones int64 [B,P+L])  (clip_whisper_model.py:407-462)."""
        x = self._llm_inputs(audio, video, prompt)
        return x, torch.ones(x.shape[0], x.shape[1], dtype=torch.long, device=x.device)

    # ------------------------------------------------------------------ forward / loss
    def _dropout_args(self):
        """lora_dropout is active in train() mode only; every training forward draws a fresh mask seed."""
        if not (self.training and self.use_lora and self.lora_dropout):
            return {"dropout": 0.0, "seed": 0}
        self._drop_step += 1
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()           # data-parallel ranks draw independent masks, as independent processes would
        return {"dropout": float(self.lora_dropout), "seed": (self._drop_step * 0x9E3779B1 + rank * 0x85EBCA6B + 12345) & 0xFFFFFFFF}

    def _prep_labels(self, labels):
        if isinstance(labels, list):
            if all(isinstance(t, torch.Tensor) for t in labels):
                labels = torch.stack(labels)
            else:
                labels = torch.tensor(labels)
        labels = labels.to(self.device)
        # :569-570 `labels[labels == pad] = -100` as one fresh tensor (no boolean-index assignment: that form syncs with the host and
        # cannot be captured in a graph)
        return torch.where(labels == self.tokenizer.pad_token_id, torch.full_like(labels, -100), labels)

    def forward(self, audio=None, video=None, prompt=None, labels=None, return_loss=True):
        """clip_whisper_model.py:489-619 -> {"loss","logits"} | {"logits"}."""
        if labels is not None and return_loss:
            try:
                labels = self._prep_labels(labels)
            except Exception as e:                                     # :541-558 dummy-loss behaviour
                logging.error(f"Failed to convert labels to tensor: {e}")
                return {"loss": torch.tensor(1.0, device=self.device, requires_grad=True), "logits": None}
        else:
            labels = None
        if self.training and labels is not None:
            x = self._llm_inputs(audio, video, prompt, S_out=labels.shape[1], keep=self.train_connectors)       # adaptive pool / interpolate (:577-585)
            logits = self.llm_engine.fwd_loss(x, labels, want_logits=True, **self._dropout_args())
            acc = self.llm_engine.acc
            loss = acc[0] / acc[1]
            if self.train_connectors:
                cps = [p for c in (self.audio_connector, self.video_connector) for p in c.parameters()]
                loss = _LoraLoss.apply(self.lora_param, self, loss, *cps)
            elif self.lora_param is not None and self.lora_param.requires_grad:
                loss = _LoraLoss.apply(self.lora_param, self, loss)
            return {"loss": loss, "logits": logits}
        x = self._llm_inputs(audio, video, prompt)
        B, S, _ = x.shape
        kc, vc = self.llm_engine.alloc_cache(B, S)
        _, logits = self.llm_engine.prefill(x, kc, vc, all_logits=True)
        if labels is None:
            return {"logits": logits}
        if labels.shape[1] > S:                                           # :586-598
            labels = labels[:, :S]
        elif labels.shape[1] < S:
            pad = torch.full((B, S - labels.shape[1]), -100, dtype=labels.dtype, device=labels.device)
            labels = torch.cat([labels, pad], dim=1)
        _, acc = ops.ce_fwd(logits, labels.contiguous())
        return {"loss": acc[0] / acc[1], "logits": logits}

    __call__ = forward

    # ------------------------------------------------------------------ generation
    @torch.no_grad()
    def generate(self, audio=None, video=None, prompt=None, pixel_values=None, max_new_tokens=100, do_sample=False,
                 temperature=1.0, top_p=0.9, max_length=None, top_k=50, seed=None, num_beams=1, length_penalty=1.0, early_stopping=False,
                 return_sequence_scores=False, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, sequence_bias=None,
                 bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, hotwords=None, hotword_bias=0.0,
                 return_token_scores=False, num_return_sequences=1):
        """clip_whisper_model.py:1240-1348 -> GenerationMixin greedy search, or with do_sample=True its sampling: temperature -> top_k
        (HF's GenerationConfig default 50; 0 = off) -> top_p -> one draw per row on the device (ops.sample_rows).  seed=None draws the
        seed from torch's default CPU generator, so torch.manual_seed makes a sampled run repeat; row b draws with seed + b.
        With do_sample=False, temperature / top_k / top_p are ignored.  Returns NEW tokens only [B, <=max_new_tokens].
        num_beams > 1: HF's beam search (see _beam_search; length_penalty, early_stopping in {True, False, "never"} as in HF); returns the
        best hypothesis per item, padded with pad_token_id, and with return_sequence_scores=True also HF's sequences_scores [B].
        repetition_penalty (> 0, 1.0 = off), no_repeat_ngram_size (0 = off) and min_new_tokens are HF's logits processors of those names, in
        every mode, applied on the device (ops.logits_process) to a row's generated tokens, which is all HF's processors see with
        inputs_embeds: on the logits before the argmax or the sampling chain, and in beam search on the log-probabilities (log-softmax
        first, as HF's _beam_search does).  With the three defaults nothing is launched.
        sequence_bias ({tuple of ids: float} or [[ids, float], ...]), bad_words_ids ([[ids], ...]), suppress_tokens and begin_suppress_tokens
        (lists of ids) are HF's keywords of those names, in the same launch and in HF's order: sequence bias, repetition penalty, n-gram
        ban, bad words, min_new_tokens, suppress, begin-suppress (the first generated token, HF's begin_index 0 with inputs_embeds).  Their
        device tables are built once per call (ops.logits_bias_tables; its capacities are refused by name); with all of them None nothing
        new is launched or allocated.  The 1024-token limit of the older processors also holds when a sequence has more than one token.
        hotwords: a list of strings boosted by hotword_bias (contextual biasing): each is tokenised with and without a leading space and
        every prefix of each tokenisation becomes a sequence_bias entry (hotword_sequence_bias below).  HF considers a sequence of L tokens
        only once L tokens have been generated, so token k of a hotword is not boosted when the word starts the utterance.
        return_token_scores=True returns a GenerateOutput (sequences, sequences_scores, token_scores, token_entropy): the log-probability
        of every returned token, HF's compute_transition_scores, computed at the token step (ops.row_scores; no second prefill), 0.0 after
        a row's EOS.  Greedy: log-softmax of the processed logits at the argmax (normalize_logits=True).  Sampled: the draw's
        log-probability under the distribution it was drawn from, after temperature, top_k and top_p (ops.sample_rows); token_entropy is
        that of the UNTRUNCATED distribution, softmax(processed logits / temperature).  Beam search: each token's log-probability as the
        beam scorer added it (processed, with processors on), carried through the beam reorderings; sequences_scores as HF.
        num_return_sequences=n: HF's keyword: rows [B*n, L], item-major; beam search returns the n best hypotheses of each item, best
        first (n <= num_beams); sampling draws n sequences per clip (encoders and connectors run once per clip; the result equals a call
        on the clips repeated n times); greedy decoding with n > 1 is a ValueError, as in HF.  With both at their defaults nothing new
        is launched or allocated and the return value is unchanged."""
        if video is None and pixel_values is not None:
            video = pixel_values
        if max_new_tokens is None:
            max_new_tokens = max_length if max_length is not None else 100
        if int(num_beams) != num_beams or num_beams < 1:
            raise ValueError(f"num_beams must be a positive integer, got {num_beams}")
        if num_beams > 1:
            if do_sample:
                raise NotImplementedError("beam sampling (do_sample=True with num_beams > 1) is not supported")
            if num_beams > ops.BEAM_MAX_BEAMS:
                raise ValueError(f"num_beams must be at most {ops.BEAM_MAX_BEAMS}, got {num_beams}")
            if early_stopping not in (True, False, "never"):
                raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
        elif return_sequence_scores:
            raise ValueError("return_sequence_scores needs num_beams > 1 (HF returns sequences_scores for beam search only)")
        n_ret = num_return_sequences
        if isinstance(n_ret, bool) or not isinstance(n_ret, numbers.Integral) or n_ret < 1:
            raise ValueError(f"num_return_sequences must be a positive integer, got {n_ret!r}")
        n_ret = int(n_ret)
        if num_beams > 1 and n_ret > num_beams:
            raise ValueError(f"num_return_sequences ({n_ret}) has to be smaller or equal to num_beams ({num_beams})")
        if num_beams == 1 and not do_sample and n_ret > 1:
            raise ValueError(f"greedy decoding cannot return {n_ret} sequences: num_return_sequences > 1 needs do_sample=True or num_beams > 1")
        if do_sample:
            ops.check_sampling(temperature, top_k, top_p)
            if seed is None:
                seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        proc = None
        if ops.check_logits_processors(repetition_penalty, no_repeat_ngram_size, min_new_tokens):
            if max_new_tokens > ops.LOGITS_PROCESS_MAX_HISTORY:
                raise ValueError(f"repetition_penalty / no_repeat_ngram_size / min_new_tokens support at most {ops.LOGITS_PROCESS_MAX_HISTORY} "
                                 f"new tokens, got max_new_tokens = {max_new_tokens}")
            proc = (float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens))
        if hotwords:
            sequence_bias = hotword_sequence_bias(self.tokenizer, hotwords, hotword_bias, sequence_bias)
        tables = {}
        if not (sequence_bias is None and bad_words_ids is None and suppress_tokens is None and begin_suppress_tokens is None):
            tables = ops.logits_bias_tables(sequence_bias, bad_words_ids, suppress_tokens, begin_suppress_tokens, vocab=self.cfg.llama.vocab,
                                            eos=self.eos_token_id, device=self.device)
        # the row history feeds the three older processors and sequences of more than one token
        need_hist = bool(proc) or any(isinstance(t, ops.SequenceTable) and t.max_len > 1 for t in tables.values())
        if need_hist and max_new_tokens > ops.LOGITS_PROCESS_MAX_HISTORY:
            raise ValueError(f"sequence_bias / bad_words_ids with sequences of more than one token support at most "
                             f"{ops.LOGITS_PROCESS_MAX_HISTORY} new tokens, got max_new_tokens = {max_new_tokens}")
        if tables and not proc:
            proc = (1.0, 0, 0)
        original = self.modality
        if audio is not None and video is not None:
            self.modality = "both"
        elif audio is not None:
            self.modality = "audio"
        elif video is not None:
            self.modality = "video"
        try:
            x = self._llm_inputs(audio, video, prompt)
        finally:
            self.modality = original
        if num_beams > 1:
            return self._beam_search(x, max_new_tokens, int(num_beams), float(length_penalty), early_stopping, return_sequence_scores, proc,
                                     tables, need_hist, n_ret=n_ret, token_scores=bool(return_token_scores))
        if n_ret > 1:
            x = x.repeat_interleave(n_ret, dim=0)                   # after the encoders and connectors, which ran once per clip
        eng = self.llm_engine
        B, S, _ = x.shape
        kc, vc = eng.alloc_cache(B, S + max_new_tokens)
        logits, _ = eng.prefill(x, kc, vc)
        eos, pad = self.eos_token_id, self.tokenizer.pad_token_id
        unfinished = torch.ones(B, dtype=torch.bool, device=x.device)
        out = []
        row_seeds = torch.arange(B, dtype=torch.int32, device=x.device) if do_sample else None
        # the processors' history: row b's generated tokens (pad after its EOS, as HF feeds them); the kernel itself appends the last token
        hist = torch.full((B, max_new_tokens), pad, dtype=torch.int64, device=x.device) if need_hist else None
        nxt = None
        tok_lp, tok_ent = [], []
        for step in range(max_new_tokens):
            if proc:
                ops.logits_process(logits, hist, step, *proc, eos=eos, append=nxt if need_hist else None, **tables)
            if return_token_scores:
                alive = unfinished.clone()                          # rows that still choose a token at this step
            if do_sample:
                nxt = ops.sample_rows(logits, temperature, top_k, top_p, seed, step, unfinished=unfinished if eos is not None else None,
                                      eos=eos, pad=pad, row_seeds=row_seeds, return_logprob=bool(return_token_scores))
                if return_token_scores:
                    nxt, lp = nxt                                   # 0 for finished rows already
                    ent = ops.row_scores(logits, nxt, temperature, entropy=True)[1]
            else:
                nxt = ops.argmax_rows(logits)
                if return_token_scores:
                    lp, ent = ops.row_scores(logits, nxt, entropy=True)
                    lp = torch.where(alive, lp, torch.zeros_like(lp))
                if eos is not None:
                    nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
                    unfinished = unfinished & (nxt != eos)
            out.append(nxt)
            if return_token_scores:
                tok_lp.append(lp)
                tok_ent.append(torch.where(alive, ent, torch.zeros_like(ent)))
            if step + 1 == max_new_tokens or (eos is not None and not bool(unfinished.any())):
                break
            logits = eng.decode_step(nxt, S + step, kc, vc)
        if return_token_scores:
            return GenerateOutput(torch.stack(out, dim=1), None, torch.stack(tok_lp, dim=1), torch.stack(tok_ent, dim=1))
        return torch.stack(out, dim=1)

    def _beam_search(self, x, max_new_tokens, nb, length_penalty, early_stopping, return_scores, proc=None, tables=None, need_hist=True,
                     n_ret=1, token_scores=False):
        """GenerationMixin._beam_search (transformers 5.x, generation/utils.py) for inputs_embeds x [B, S, d]: decoder_prompt_len = 0, so a
        hypothesis of n tokens (its EOS included) is normalised by n ** length_penalty, and max_length = max_new_tokens.  Per token step:
        the B*nb-row decode step, ops.beam_topk (log_softmax + _get_top_k_continuations, k = 2*nb), HF's bookkeeping
        (_get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic,
        _beam_search_has_unfinished_sequences) restated on small device tensors, and ops.kv_gather_rows reordering only the generated
        positions [S, S + step): every beam of an item shares the prefix [0, S), which is copied once from the B-row prefill cache.
        Equal scores keep candidate order (stable sorts where HF calls torch.topk).  One host sync per step, for the stopping test.
        B*nb <= 16 rows take the fused bf16 token step (LlamaEngine.decode_is_fused); more rows take the general step.
        proc = (repetition_penalty, no_repeat_ngram_size, min_new_tokens): HF runs its logits processors between the log_softmax and the
        addition of the running beam scores, on running_sequences[:, :, :cur]; ops.logits_process(log_softmax=True) does both on the
        B*nb rows and beam_topk then takes the rows as log-probabilities.  tables: generate()'s prepared sequence_bias / bad_words_ids /
        suppress_tokens / begin_suppress_tokens, for the same launch; need_hist: whether any of it reads running_sequences.
        n_ret: the n best finished hypotheses of each item are returned, rows [B*n_ret, L] item-major, best first (HF's
        num_return_sequences).  token_scores: every candidate's own log-probability, read from the row it came from (the processed
        log-probability with proc; logit - logsumexp of the raw row otherwise, ops.row_scores), and that row's entropy are carried in
        [B, nb, N] tensors through the gathers that reorder the sequences; returns a GenerateOutput.  Never derived as
        topk_lp - running_scores[parent]: that difference loses the low bits of a long hypothesis."""
        eng = self.llm_engine
        dev = x.device
        B, S, _ = x.shape
        R, k, N = B * nb, 2 * nb, max_new_tokens
        eos, pad = self.eos_token_id, self.tokenizer.pad_token_id
        kc0, vc0 = eng.alloc_cache(B, S)
        logits, _ = eng.prefill(x, kc0, vc0)
        kc, vc = eng.alloc_cache(R, S + N)
        ops.kv_gather_rows(kc0, vc0, kc, vc, torch.arange(R, device=dev, dtype=torch.int32) // nb, 0, S)    # prefix broadcast
        del kc0, vc0
        logits = logits.repeat_interleave(nb, dim=0)                # step 0: every beam of an item sees the prefill logits
        NEG = -1.0e9
        running_seq = torch.full((B, nb, N), pad, dtype=torch.int64, device=dev)
        sequences = running_seq.clone()
        running_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
        running_scores[:, 1:] = NEG
        beam_scores = torch.full((B, nb), NEG, dtype=torch.float32, device=dev)
        lengths = torch.zeros((B, nb), dtype=torch.int64, device=dev)             # generated length of each finished hypothesis
        is_sent_finished = torch.zeros((B, nb), dtype=torch.bool, device=dev)
        if token_scores:
            running_tok_lp = torch.zeros((B, nb, N), dtype=torch.float32, device=dev)
            running_ent, tok_lp, tok_ent = running_tok_lp.clone(), running_tok_lp.clone(), running_tok_lp.clone()
        unsatisfied = torch.ones((B, 1), dtype=torch.bool, device=dev)
        top_mask = torch.arange(k, device=dev) < nb
        offset = (torch.arange(B, device=dev, dtype=torch.int32) * nb)[:, None]
        done_host = torch.zeros(1, dtype=torch.bool).pin_memory()
        ev = torch.cuda.Event()
        for cur in range(N):
            # _get_top_k_continuations
            if proc:
                ops.logits_process(logits, running_seq.view(R, N) if need_hist else None, cur, *proc, eos=eos, log_softmax=True, **(tables or {}))
            topk_lp, topk_beam, topk_tok = ops.beam_topk(logits, running_scores.view(-1), nb, k, logprobs=bool(proc))
            topk_seq = torch.gather(running_seq, 1, topk_beam.long()[:, :, None].expand(B, k, N)).clone()
            topk_seq[:, :, cur] = topk_tok
            topk_parent = topk_beam + offset
            if token_scores:
                # the candidates' own log-probabilities and their rows' entropies, from the B*nb rows beam_topk selected from
                norm, row_ent = ops.row_scores(logits, None, entropy=True, logprobs=bool(proc))    # norm: -logsumexp (0 for log-probabilities)
                cand_lp = logits[topk_parent.long(), topk_tok]
                if not proc:
                    cand_lp = cand_lp + norm[topk_parent.long()]
                bidx = topk_beam.long()[:, :, None].expand(B, k, N)
                topk_tok_lp = torch.gather(running_tok_lp, 1, bidx).clone()
                topk_tok_lp[:, :, cur] = cand_lp
                topk_ent = torch.gather(running_ent, 1, bidx).clone()
                topk_ent[:, :, cur] = row_ent[topk_parent.long()]
            # stopping criteria: EOS, or max_length reached
            if cur + 1 >= N:
                hits = torch.ones((B, k), dtype=torch.bool, device=dev)
            elif eos is not None:
                hits = topk_tok == eos
            else:
                hits = torch.zeros((B, k), dtype=torch.bool, device=dev)
            # _get_running_beams_for_next_iteration
            topk_running_lp = topk_lp + hits.to(torch.float32) * NEG
            nxt = torch.sort(topk_running_lp, dim=1, descending=True, stable=True)[1][:, :nb]
            running_seq = torch.gather(topk_seq, 1, nxt[:, :, None].expand(B, nb, N))
            running_scores = torch.gather(topk_running_lp, 1, nxt)
            parent = torch.gather(topk_parent, 1, nxt)
            if token_scores:
                running_tok_lp = torch.gather(topk_tok_lp, 1, nxt[:, :, None].expand(B, nb, N))
                running_ent = torch.gather(topk_ent, 1, nxt[:, :, None].expand(B, nb, N))
            # _update_finished_beams
            just = hits & top_mask[None, :]
            fin_lp = topk_lp / ((cur + 1) ** length_penalty)
            full = torch.all(is_sent_finished, dim=-1, keepdim=True) & (early_stopping is True)
            fin_lp += full.to(torch.float32) * NEG
            fin_lp += (~unsatisfied).to(torch.float32) * NEG
            fin_lp += (~just) * NEG
            m_scores = torch.cat((beam_scores, fin_lp), dim=1)
            sel = torch.sort(m_scores, dim=1, descending=True, stable=True)[1][:, :nb]
            sequences = torch.gather(torch.cat((sequences, topk_seq), dim=1), 1, sel[:, :, None].expand(B, nb, N))
            beam_scores = torch.gather(m_scores, 1, sel)
            lengths = torch.gather(torch.cat((lengths, torch.full((B, k), cur + 1, dtype=torch.int64, device=dev)), dim=1), 1, sel)
            is_sent_finished = torch.gather(torch.cat((is_sent_finished, just), dim=1), 1, sel)
            if token_scores:
                tok_lp = torch.gather(torch.cat((tok_lp, topk_tok_lp), dim=1), 1, sel[:, :, None].expand(B, nb, N))
                tok_ent = torch.gather(torch.cat((tok_ent, topk_ent), dim=1), 1, sel[:, :, None].expand(B, nb, N))
            if cur + 1 >= N:                                        # every candidate hit max_length: HF's loop ends here
                break
            # _check_early_stop_heuristic at cur_len = cur + 1, then _beam_search_has_unfinished_sequences
            if early_stopping == "never" and length_penalty > 0.0:
                best_len = N
            else:
                best_len = cur + 1
            best_running = running_scores[:, :1] / (best_len ** length_penalty)
            worst_finished = torch.where(is_sent_finished, torch.min(beam_scores, dim=1, keepdim=True)[0], NEG)
            unsatisfied = unsatisfied & torch.any(best_running > worst_finished, dim=-1, keepdim=True)
            done = ~(torch.any(unsatisfied) & ~(torch.all(is_sent_finished) & (early_stopping is True)) & ~torch.all(hits))
            done_host.copy_(done.view(1), non_blocking=True)
            ev.record()
            # the next token step is queued before the host waits on the stopping test (only the small copy above is awaited)
            ops.kv_gather_rows(kc, vc, kc, vc, parent.view(-1).to(torch.int32), S, S + cur)
            logits = eng.decode_step(running_seq[:, :, cur].reshape(-1), S + cur, kc, vc)
            ev.synchronize()
            if bool(done_host[0]):
                break
        L = int(lengths[:, :n_ret].max())
        out = sequences[:, :n_ret, :L].reshape(B * n_ret, L)
        scores = beam_scores[:, :n_ret].reshape(B * n_ret)
        if token_scores:
            return GenerateOutput(out, scores, tok_lp[:, :n_ret, :L].reshape(B * n_ret, L), tok_ent[:, :n_ret, :L].reshape(B * n_ret, L))
        return (out, scores) if return_scores else out
