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
  * lora_target_modules (default None = q_proj, k_proj, v_proj, o_proj, the reference's own list): any non-empty subset of those four and
    gate_proj, up_proj, down_proj, or "all-linear" (peft's name) for all seven.  An adapter on an MLP projection trains, evaluates and
    generates like the others, but keeps generate()'s token steps off the fused path until merge_lora() folds it (see generate()).
  * train_connectors=True (default False) trains the two modality connectors with the encoders frozen: the reference's freeze_encoders=False
    gradient (clip_whisper_model.py:1096-1106,1136-1146) restricted to the four connector tensors, which does not depend on whether the
    encoders receive one too.  connector_type "simple", precision fp32 | bf16, use_lora=True.
  * modality_dropout_audio / modality_dropout_video (default 0 = off) and the modality_mask keyword of forward() / encode() / generate() are
    additions: one mode per clip (both | audio only | video only) at the geometry of the two-stream call, drawn per step in train() mode or
    given by the caller (see forward()).  Without them the model launches what it launched.
  * label_smoothing / z_loss (default 0 = off) are additions: the objective of the training forward only (see the constructor); eval() and
    everything built on it keep the plain cross entropy.  Without them the model launches what it launched.
"""
from __future__ import annotations

import logging
import os
import types

import torch

from . import lib as L
from . import ops
from .arch import LORA_MLP_MODULES, LORA_MODULES, ModelCfg, lora_state_key, parse_lora_state_key, parse_lora_targets, resolve_arch
from .connector import ModalityConnector, create_modality_connector
from .engine import ClipEngine, LlamaEngine, WhisperEngine
from .generation import GenerateOutput, beam_search, hotword_sequence_bias, parse_arguments, shares_prefix, token_loop  # noqa: F401  (the first and third are re-exported)
from .tokenizer import load_tokenizer


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


MODALITY_MODES = {"both": 0, "audio": 1, "video": 2}      # AVLLM_MODE_* of include/avllm.h


def parse_modality_mask(mask, B, device=None):
    """A modality_mask as an int32 tensor [B]: a list / tuple / CPU tensor of 0 | 1 | 2 or "both" | "audio" | "video" is checked (length B, values
    in range) and moved to `device` (None: left on the CPU); an int32 device tensor [B] is taken as given."""
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        if mask.dtype != torch.int32 or mask.dim() != 1 or mask.shape[0] != B:
            raise ValueError(f"modality_mask on the device must be int32 [{B}], got {mask.dtype} {tuple(mask.shape)}")
        return mask.contiguous()
    if isinstance(mask, torch.Tensor):
        if mask.dim() != 1 or mask.dtype.is_floating_point or mask.dtype == torch.bool:
            raise ValueError(f"modality_mask must be a 1-d integer tensor, got {mask.dtype} {tuple(mask.shape)}")
        vals = mask.tolist()
    elif isinstance(mask, (list, tuple)):
        vals = list(mask)
    else:
        raise ValueError(f"modality_mask must be a list or a tensor with one entry per clip, got {type(mask).__name__}")
    if len(vals) != B:
        raise ValueError(f"modality_mask has {len(vals)} entries for a batch of {B} clips (one per clip, not per beam or returned sequence)")
    out = []
    for i, m in enumerate(vals):
        if isinstance(m, str):
            if m not in MODALITY_MODES:
                raise ValueError(f"modality_mask[{i}] = {m!r}: must be both | audio | video (or 0 | 1 | 2)")
            m = MODALITY_MODES[m]
        if isinstance(m, bool) or not isinstance(m, int) or m not in (0, 1, 2):
            raise ValueError(f"modality_mask[{i}] = {m!r}: must be 0 (both) | 1 (audio) | 2 (video)")
        out.append(m)
    t = torch.tensor(out, dtype=torch.int32)
    return t if device is None else t.to(device)


class ClipWhisperModel:
    def __init__(self, llm_path="meta-llama/Llama-2-7b-hf", whisper_model="openai/whisper-small",
                 clip_model="openai/clip-vit-base-patch16", device="cuda", use_fp16=False, use_4bit=False, use_lora=True,
                 lora_r=16, lora_alpha=32, lora_dropout=0.05, freeze_encoders=True, freeze_llm=False, modality="both",
                 max_seq_len=256, fusion_scale=0.5, connector_type="simple", _provided_tokenizer=None, _provided_llm=None,
                 _provided_whisper=None, _provided_clip=None, *, precision=None, config: ModelCfg | None = None,
                 weights: dict | None = None, seed: int = 0, synthetic_weights: bool = False, decode_weights: str = "bf16",
                 train_connectors: bool = False, kv_cache: str = "bf16", lora_target_modules=None,
                 modality_dropout_audio: float = 0.0, modality_dropout_video: float = 0.0,
                 label_smoothing: float = 0.0, z_loss: float = 0.0):
        if use_4bit:
            raise NotImplementedError("use_4bit (bitsandbytes nf4) is out of scope of the MI355X hot path (SURVEY.md §8)")
        if not freeze_encoders:
            raise NotImplementedError("freeze_encoders=False is not supported: the hot path trains LoRA only (SURVEY.md fact 4)")
        if modality not in ("audio", "video", "both"):
            raise ValueError(f"modality must be audio|video|both, got {modality}")
        # modality dropout (AV-HuBERT's training recipe; not in the reference): in train() mode every clip of a two-stream call loses its audio
        # with probability modality_dropout_audio or its video with modality_dropout_video, never both; drawn on the device per step
        # (ops.modality_draw) and applied by the fusion (ops.fuse_pool_rows).  The encoders still run on every clip.  Its effect on WER is
        # not measured.
        for nm, p in (("modality_dropout_audio", modality_dropout_audio), ("modality_dropout_video", modality_dropout_video)):
            if not isinstance(p, (int, float)) or isinstance(p, bool) or not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"{nm} must be a probability in [0, 1], got {p!r}")
        if float(modality_dropout_audio) + float(modality_dropout_video) > 1.0:
            raise ValueError(f"modality_dropout_audio + modality_dropout_video must be at most 1 (a clip never loses both streams), got "
                             f"{modality_dropout_audio} + {modality_dropout_video}")
        if modality != "both" and (modality_dropout_audio or modality_dropout_video):
            nm = "modality_dropout_audio" if modality_dropout_audio else "modality_dropout_video"
            raise ValueError(f"{nm}={modality_dropout_audio or modality_dropout_video} needs modality='both', got modality={modality!r}: "
                             f"there is no second stream to fall back on")
        self.modality_dropout_audio, self.modality_dropout_video = float(modality_dropout_audio), float(modality_dropout_video)
        # label smoothing and the PaLM z-loss (not in the reference, whose trainer takes HF's loss as it is): the training forward's objective is
        # (1 - label_smoothing) nll + label_smoothing (lse - mean logit) + z_loss lse^2 per scored token (avllm_ce_smooth_fwd).  The eval()
        # forward keeps the plain cross entropy, so validation losses compare across runs with and without them.  Effect on WER not measured.
        for nm, p in (("label_smoothing", label_smoothing), ("z_loss", z_loss)):
            if not isinstance(p, (int, float)) or isinstance(p, bool):
                raise ValueError(f"{nm} must be a number, got {p!r}")
        self.label_smoothing, self.z_loss = ops.check_loss_options(label_smoothing, z_loss)
        self.last_modality_modes = None            # int32 [B] device buffer of the last call that used per-clip modes, else None
        self.last_modality_seed = None             # the by-value seed of that call's draw (None: no draw, or the seed came from device memory)
        self._mode_bufs = {}
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
        if lora_target_modules is not None and not use_lora:
            raise ValueError(f"lora_target_modules={lora_target_modules!r} together with use_lora=False: there are no adapters to place")
        lora_targets = parse_lora_targets(lora_target_modules) if lora_target_modules is not None else None
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
        # kv_cache="fp8": generate() (greedy, sampled, beam) keeps K and V as e4m3 codes with one E8M0 exponent per 32 elements of a cache row
        # (33/64 of the bf16 bytes) and its token steps attend over that form directly: K stored after RoPE, V as projected, a token's own row
        # as stored.  Goes with the fused token step (at most 16 rows, B * num_beams in beam search); more rows get the bf16 cache.  The
        # prefill's logits, so the first token, are those of "bf16"; forward() keeps its bf16 cache.  A runtime choice: not saved with the model.
        if kv_cache not in ("bf16", "fp8"):
            raise ValueError(f"kv_cache must be bf16|fp8, got {kv_cache!r}")
        if kv_cache == "fp8" and precision == "fp32":
            raise ValueError("kv_cache='fp8' needs precision bf16 or fp8, not precision='fp32' (the fp8 cache goes with the bf16 fused token step)")
        self.kv_cache = kv_cache
        self.train_connectors = bool(train_connectors)
        if self.train_connectors:
            if connector_type != "simple":
                raise NotImplementedError(f"train_connectors=True supports connector_type='simple' only, got {connector_type!r}")
            if precision == "fp8":
                raise NotImplementedError("train_connectors=True supports precision fp32 | bf16, not fp8")
            if not use_lora:
                raise ValueError("train_connectors=True needs use_lora=True: the LoRA backward pass is the only LLM backward pass in the library")
        if precision == "fp8" and lora_targets is not None and any(nm in LORA_MLP_MODULES for nm in lora_targets):
            raise NotImplementedError("precision='fp8' with lora_target_modules on " + ", ".join(nm for nm in lora_targets if nm in LORA_MLP_MODULES) +
                                      " is not implemented: the fp8 training forward takes adapters on q_proj, k_proj, v_proj and o_proj only")
        self.dtype = torch.float32 if precision == "fp32" else torch.bfloat16
        self.training = True
        self._drop_step = 0
        self._seed = int(seed or 0)

        cfg, W = resolve_arch(llm_path, whisper_model, clip_model, config, weights, seed, lora_r, lora_alpha, use_lora,
                              _provided_llm, _provided_whisper, _provided_clip, device, self.dtype, synthetic_weights, lora_targets=lora_targets)
        # the adapted modules in canonical order (a `config=` may carry its own in LoraCfg.targets); saved by save_pretrained()
        self.lora_target_modules = tuple(cfg.lora.targets) if use_lora else ()
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
                                      training=True, fp8=self.fp8, decode_fp8=decode_weights == "fp8", decode_fp4=decode_weights == "fp4",
                                      kv_fp8=kv_cache == "fp8")
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
                sd[lora_state_key(i, mod, ab)] = v.detach().clone()
        return sd

    def load_state_dict(self, sd, strict=False):
        if self.llm_engine.merged and any(".lora_A." in k or ".lora_B." in k for k in sd):      # refused before anything is loaded
            raise RuntimeError("load_state_dict(): LoRA tensors cannot be loaded after merge_lora() folded the adapters into the LLM weights")
        a = {k.split("audio_connector.")[1]: v for k, v in sd.items() if "audio_connector." in k}
        v_ = {k.split("video_connector.")[1]: v for k, v in sd.items() if "video_connector." in k}
        if a:
            self.audio_connector.load_state_dict(a)
        if v_:
            self.video_connector.load_state_dict(v_)
        lora = {}
        for k, t in sd.items():
            if parse_lora_state_key(k) is not None:
                i, mod, ab = parse_lora_state_key(k)
                if self.use_lora and mod not in self.lora_target_modules:      # refused before anything of the adapters is loaded
                    known = "" if mod in LORA_MODULES else " (not a module name this build knows)"
                    raise ValueError(f"load_state_dict(): {k} is a LoRA tensor of {mod}{known}, which this model does not adapt "
                                     f"(lora_target_modules = {', '.join(self.lora_target_modules)})")
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
                   lora_target_modules=list(self.lora_target_modules) if self.use_lora else None,
                   audio_dim=self.audio_dim, video_dim=self.video_dim, llm_dim=self.llm_dim)
        json.dump(cfg, open(os.path.join(output_dir, "config.json"), "w"), indent=2)
        torch.save(cfg, os.path.join(output_dir, "config.pt"))
        if self.use_lora:
            os.makedirs(os.path.join(output_dir, "llm"), exist_ok=True)
            torch.save({k: v for k, v in self.state_dict().items() if "lora_" in k}, os.path.join(output_dir, "llm", "adapter_model.pt"))

    def merge_lora(self):
        """peft's merge_and_unload() for decoding: W' = W + (alpha/r) B.A on every adapted projection of every layer, once (LlamaEngine.merge_lora), so that
        generate() and an eval forward() run the adapter-free kernels.  For good: the model is set to eval, and a training forward and
        load_state_dict with LoRA tensors raise afterwards; state_dict() and save_pretrained() still hold the adapters as loaded."""
        self.eval()
        self.llm_engine.merge_lora()
        return self

    def merged_llm_state_dict(self):
        """The whole LLM after merge_lora() as HuggingFace-named tensors (LlamaEngine.merged_llm_state_dict)."""
        return self.llm_engine.merged_llm_state_dict()

    @classmethod
    def from_pretrained(cls, model_dir, tokenizer=None, merge_lora=False, **kwargs):
        """clip_whisper_model.py:821-864.  The reference's own pair is not closed: its save_pretrained writes `config.pt` / `config.json` while its
        from_pretrained demands `model_config.json` (and `whisper/`, `clip/` directories that are only written with freeze_encoders=False), so it
        cannot reload what it saved.  This one reloads what save_pretrained above wrote -- connectors, adapters, the saved settings -- on top of
        base checkpoints named by the usual constructor keywords (`llm_path=`, `whisper_model=`, `clip_model=`, or `config=` + `synthetic_weights=`).
        merge_lora=True: merge_lora() once the adapters are loaded."""
        import json
        if not os.path.exists(model_dir):
            raise ValueError(f"Model directory {model_dir} does not exist")
        cfg_path = os.path.join(model_dir, "config.json")
        if not os.path.exists(cfg_path):
            raise ValueError(f"Model config {cfg_path} does not exist")
        cfg = json.load(open(cfg_path))
        for k in ("modality", "max_seq_len", "fusion_scale", "use_lora", "lora_r", "lora_alpha", "connector_type", "lora_target_modules"):
            if k in cfg:
                kwargs.setdefault(k, cfg[k])
        if not kwargs.get("use_lora", True):
            kwargs.pop("lora_target_modules", None)               # a directory saved with adapters, reloaded without them
        model = cls(_provided_tokenizer=tokenizer, **kwargs)
        model.audio_connector.load_state_dict(torch.load(os.path.join(model_dir, "audio_connector.pt"), map_location=model.device, weights_only=True))
        model.video_connector.load_state_dict(torch.load(os.path.join(model_dir, "video_connector.pt"), map_location=model.device, weights_only=True))
        adapters = os.path.join(model_dir, "llm", "adapter_model.pt")
        if model.use_lora and os.path.exists(adapters):
            model.load_state_dict(torch.load(adapters, map_location="cpu", weights_only=True))
        if merge_lora:
            model.merge_lora()
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
        _, _, _, _, S, B, _ = self._conn_geo
        return self._static("dx", (B, S, self.llm_dim))

    def connector_backward(self, accumulate=False):
        """dx_embeds -> fuse / pool adjoint -> the two weight gradients and bias gradients, written into conn_g (overwritten, not
        accumulated).  The connectors' INPUT gradient is not formed: the encoders are frozen.  An input that was absent in the forward
        leaves its connector's gradient as zeros.
        accumulate=True (a micro-step of a gradient-accumulation window): the gradients are ADDED to conn_g (avllm_gemm_wgrad_acc; whoever
        opens the window zeroes it) and an absent input adds nothing; da / dv stay per-call temporaries."""
        Ta, Tv, P, Lc, S, B, modes = self._conn_geo
        D = self.llm_dim
        da = self._static("da", (B, Ta, D)) if Ta else None
        dv = self._static("dv", (B, Tv, D)) if Tv else None
        if modes is not None:               # per-clip modes: a clip's unused stream gets zero rows, which add nothing to dW / db below
            ops.fuse_pool_rows_bwd(self._dx_embeds_buffer(), modes, Ta, Tv, P, Lc, self.fusion_scale, da=da, dv=dv)
        else:
            ops.fuse_pool_bwd(self._dx_embeds_buffer(), Ta, Tv, P, Lc, self.fusion_scale, da=da, dv=dv)
        gWa, gba, gWv, gbv = self.connector_grad_views()
        for dy, conn, gW, gb in ((da, self.audio_connector, gWa, gba), (dv, self.video_connector, gWv, gbv)):
            if accumulate:
                if dy is not None:
                    ops.gemm_wgrad_acc(dy.view(-1, D), conn.saved_input, gW, gb)
            elif dy is None:
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

    def _modes_for(self, modality_mask, audio, video, draw_seed, seed_dev):
        """The per-clip mode buffer of this call (int32 [B] on the device), or None for the default path.  Before the encoders run, so that a
        bad mask costs nothing.  A draw happens in train() mode on a two-stream call when a dropout probability is set: ops.modality_draw into a
        static buffer (one per batch size: a captured step replays the launch on the same address), with the mask as mode_in."""
        both = self.modality == "both" and audio is not None and video is not None
        if modality_mask is not None and not both:
            raise ValueError("modality_mask needs a call with both audio and video on a modality='both' model: a call on one stream has "
                             "nothing to choose between")
        draw = self.training and both and (self.modality_dropout_audio > 0.0 or self.modality_dropout_video > 0.0)
        self.last_modality_modes = self.last_modality_seed = None
        if modality_mask is None and not draw:
            return None
        B = audio.shape[0]
        modes = parse_modality_mask(modality_mask, B, self.device) if modality_mask is not None else None
        if draw:
            buf = self._mode_bufs.get(B)
            if buf is None:
                buf = self._mode_bufs[B] = torch.zeros(B, dtype=torch.int32, device=self.device)
            if seed_dev is None and draw_seed is None:
                draw_seed = self._next_seed()
            self.last_modality_seed = None if seed_dev is not None else int(draw_seed)
            modes = ops.modality_draw(B, self.modality_dropout_audio, self.modality_dropout_video, seed=draw_seed or 0, seed_dev=seed_dev,
                                      mode_in=modes, out=buf)
        self.last_modality_modes = modes
        return modes

    def _llm_inputs(self, audio, video, prompt, S_out=None, keep=False, modality_mask=None, draw_seed=None, seed_dev=None):
        """keep (train_connectors=True, training forward): the connectors keep the rows they project and the fusion geometry is recorded,
        which is all connector_backward() needs -- no second encoder pass.
        modality_mask / a modality-dropout draw (_modes_for; draw_seed by value or seed_dev, the address of a device word): the fusion
        takes one mode per clip (ops.fuse_pool_rows) at the geometry of the two-stream call; without either it is ops.fuse_pool as ever."""
        modes = self._modes_for(modality_mask, audio, video, draw_seed, seed_dev)
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
            self._conn_geo = (a.shape[1] if a is not None else 0, v.shape[1] if v is not None else 0, P, Lc, S, B, modes)
        if modes is not None:
            return ops.fuse_pool_rows(a, v, pe, modes, Lc, S, self.fusion_scale, self.llm_dim, B)
        return ops.fuse_pool(a, v, pe, Lc, S, self.fusion_scale, self.llm_dim, B)

    def encode(self, audio=None, video=None, prompt=None, modality_mask=None):
        """-> (inputs_embeds [B,P+L,D], attention_mask ones int64 [B,P+L])  (clip_whisper_model.py:407-462).
        modality_mask: one mode per clip, see forward()."""
        x = self._llm_inputs(audio, video, prompt, modality_mask=modality_mask)
        return x, torch.ones(x.shape[0], x.shape[1], dtype=torch.long, device=x.device)

    # ------------------------------------------------------------------ forward / loss
    def _next_seed(self):
        """The seed of the next training forward: the formula of avllm_step_state.dropout_seed on a host-side step count."""
        self._drop_step += 1
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()           # data-parallel ranks draw independent masks, as independent processes would
        return (self._drop_step * 0x9E3779B1 + rank * 0x85EBCA6B + 12345) & 0xFFFFFFFF

    def _dropout_args(self):
        """lora_dropout is active in train() mode only; every training forward draws a fresh mask seed."""
        if not (self.training and self.use_lora and self.lora_dropout):
            return {"dropout": 0.0, "seed": 0}
        return {"dropout": float(self.lora_dropout), "seed": self._next_seed()}

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

    def forward(self, audio=None, video=None, prompt=None, labels=None, return_loss=True, modality_mask=None):
        """clip_whisper_model.py:489-619 -> {"loss","logits"} | {"logits"}.
        modality_mask (not in the reference): one entry per clip of a two-stream call, 0 | "both", 1 | "audio" (video ignored), 2 | "video"
        (audio ignored), as a list or CPU tensor (checked here: length B, values in range) or an int32 device tensor [B] (taken as given;
        any value other than 1 or 2 reads as 0).  The batch keeps the two-stream geometry; a clip's ignored stream is not read by the fusion and
        may hold anything.  In train() mode with modality_dropout_audio / _video set, the clips the mask leaves at 0 are drawn per call
        (ops.modality_draw) with the seed of this forward's LoRA dropout; model.last_modality_modes holds the modes used."""
        if labels is not None and return_loss:
            try:
                labels = self._prep_labels(labels)
            except Exception as e:                                     # :541-558 dummy-loss behaviour
                logging.error(f"Failed to convert labels to tensor: {e}")
                return {"loss": torch.tensor(1.0, device=self.device, requires_grad=True), "logits": None}
        else:
            labels = None
        if self.training and labels is not None:
            if self.llm_engine.merged:
                raise RuntimeError("forward(): a training forward needs the separate adapters, which merge_lora() folded into the LLM weights")
            drop = self._dropout_args()                # first: a modality-dropout draw shares this forward's seed
            x = self._llm_inputs(audio, video, prompt, S_out=labels.shape[1], keep=self.train_connectors, modality_mask=modality_mask,
                                 draw_seed=drop["seed"] if drop["dropout"] else None)       # adaptive pool / interpolate (:577-585)
            logits = self.llm_engine.fwd_loss(x, labels, want_logits=True, label_smoothing=self.label_smoothing, z_loss=self.z_loss, **drop)
            acc = self.llm_engine.acc
            loss = acc[0] / acc[1]
            # with label smoothing or the z-loss on, "loss" is the composite objective and "nll_loss" the plain cross entropy of the same rows
            nll = {"nll_loss": self.llm_engine.loss_terms[0] / acc[1]} if (self.label_smoothing or self.z_loss) else {}
            if self.train_connectors:
                cps = [p for c in (self.audio_connector, self.video_connector) for p in c.parameters()]
                loss = _LoraLoss.apply(self.lora_param, self, loss, *cps)
            elif self.lora_param is not None and self.lora_param.requires_grad:
                loss = _LoraLoss.apply(self.lora_param, self, loss)
            return {"loss": loss, "logits": logits, **nll}
        x = self._llm_inputs(audio, video, prompt, modality_mask=modality_mask)
        B, S, _ = x.shape
        kc, vc = self.llm_engine.alloc_cache(B, S, fp8=False)
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
                 return_token_scores=False, num_return_sequences=1, share_prefix=False, modality_mask=None):
        """clip_whisper_model.py:1240-1348 -> GenerationMixin's greedy search, sampling or beam search on the fused inputs (avllm/generation.py).
        Returns NEW tokens only, int64 [B, <= max_new_tokens], pad_token_id after a row's EOS.  With every keyword at its default nothing but
        the greedy loop is launched or allocated.  video is also taken as pixel_values; max_new_tokens=None means max_length, else 100.
        do_sample, temperature, top_k, top_p, seed: HF's sampling: temperature -> top_k (HF's GenerationConfig default 50; 0 = off) -> top_p ->
          one draw per row on the device (ops.sample_rows).  seed=None draws the seed from torch's default CPU generator, so
          torch.manual_seed makes a sampled run repeat; row b draws with seed + b.  With do_sample=False the other four are ignored.
        num_beams > 1, length_penalty, early_stopping (True, False or "never", as in HF), return_sequence_scores: HF's beam search
          (generation.beam_search); returns the best hypothesis per item, padded with pad_token_id, and with return_sequence_scores=True
          also HF's sequences_scores [B].  Beam sampling (do_sample=True with it) is NotImplementedError.
        repetition_penalty (> 0, 1.0 = off), no_repeat_ngram_size (0 = off), min_new_tokens: HF's logits processors of those names, in every
          mode, applied on the device (ops.logits_process) to a row's generated tokens, which is all HF's processors see with inputs_embeds:
          on the logits before the argmax or the sampling chain, and in beam search on the log-probabilities (log-softmax first, as HF's
          _beam_search does).  With the three defaults nothing is launched.
        sequence_bias ({tuple of ids: float} or [[ids, float], ...]), bad_words_ids ([[ids], ...]), suppress_tokens, begin_suppress_tokens
          (lists of ids): HF's keywords of those names, in the same launch and in HF's order: sequence bias, repetition penalty, n-gram ban,
          bad words, min_new_tokens, suppress, begin-suppress (the first generated token, HF's begin_index 0 with inputs_embeds).  Their
          device tables are built once per call (ops.logits_bias_tables; its capacities are refused by name); with all of them None nothing
          new is launched or allocated.  The 1024-token limit of the older processors also holds when a sequence has more than one token.
        hotwords, hotword_bias: a list of strings boosted by hotword_bias (contextual biasing): each is tokenised with and without a leading
          space and every prefix of each tokenisation becomes a sequence_bias entry (generation.hotword_sequence_bias).  HF considers a sequence
          of L tokens only once L tokens have been generated, so token k of a hotword is not boosted when the word starts the utterance.
        return_token_scores=True: returns a GenerateOutput (sequences, sequences_scores, token_scores, token_entropy): the log-probability
          of every returned token, HF's compute_transition_scores, computed at the token step (ops.row_scores; no second prefill), 0.0
          after a row's EOS.  Greedy: log-softmax of the processed logits at the argmax (normalize_logits=True).  Sampled: the draw's
          log-probability under the distribution it was drawn from, after temperature, top_k and top_p (ops.sample_rows); token_entropy is
          that of the UNTRUNCATED distribution, softmax(processed logits / temperature).  Beam search: each token's log-probability as the
          beam scorer added it (processed, with processors on), carried through the beam reorderings; sequences_scores as HF.
        num_return_sequences=n: HF's keyword: rows [B*n, L], item-major; beam search returns the n best hypotheses of each item, best first
          (n <= num_beams); sampling draws n sequences per clip (encoders and connectors run once per clip; the result equals a call on the
          clips repeated n times); greedy decoding with n > 1 is a ValueError, as in HF.
        share_prefix=True: the beams of an item (num_beams > 1), or its n sampled sequences (num_return_sequences = n > 1), read ONE copy of
          the item's prefix -- the B-row cache of the prefill, which for sampling then runs on B rows, not B*n -- and keep only their own
          generated positions in a suffix cache of max_new_tokens rows (csrc/attention_decode_shared.hip): a memory saving first (B*S + R*N
          cached positions for R*(S + N)), and fewer cache bytes read per step.  The keys and values every row attends are the same; sums
          are taken in another order, so scores agree to bf16 rounding, not bit for bit.  It goes with the fused token step
          (LlamaEngine.decode_shares_prefix: at most 16 rows, bf16, head dim 64 or 128): with more rows, precision="fp32" or the fused step
          switched off, and for greedy decoding and n = 1 sampling, which have nothing to share, the keyword is accepted and the call takes
          the default path, bit-equal to share_prefix=False.
        lora_target_modules with gate_proj, up_proj or down_proj: while such an adapter is attached (not merged) every token step takes the
          general path (LlamaEngine.decode_is_fused is False): correct, but without the fused step's speed and without what goes with it --
          decode_weights="fp8" | "fp4" stream bf16 weights, kv_cache="fp8" keeps a bf16 cache, share_prefix takes the default path.  The
          remedy is merge_lora() (or from_pretrained(..., merge_lora=True)): the model is then adapter-free and takes the fused step in
          every weight and cache form.
        modality_mask: one mode per CLIP (not per beam or returned sequence) of a two-stream call, as in forward(): it acts on the fused inputs,
          before beams or n-best expand the rows, so every decoding mode, weight form and cache form takes it unchanged."""
        if video is None and pixel_values is not None:
            video = pixel_values
        eos, pad = self.eos_token_id, self.tokenizer.pad_token_id
        max_new_tokens, n_ret, sample, processors = parse_arguments(
            self.tokenizer, self.cfg.llama.vocab, eos, self.device, max_new_tokens=max_new_tokens, max_length=max_length, do_sample=do_sample,
            temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, num_beams=num_beams, early_stopping=early_stopping,
            return_sequence_scores=return_sequence_scores, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
            min_new_tokens=min_new_tokens, sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, suppress_tokens=suppress_tokens,
            begin_suppress_tokens=begin_suppress_tokens, hotwords=hotwords, hotword_bias=hotword_bias, num_return_sequences=num_return_sequences,
            share_prefix=share_prefix)
        original = self.modality
        if audio is not None and video is not None:
            self.modality = "both"
        elif audio is not None:
            self.modality = "audio"
        elif video is not None:
            self.modality = "video"
        try:
            x = self._llm_inputs(audio, video, prompt, modality_mask=modality_mask)
        finally:
            self.modality = original
        if num_beams > 1:
            return beam_search(self.llm_engine, x, eos, pad, max_new_tokens, int(num_beams), float(length_penalty), early_stopping,
                               processors, n_ret=n_ret, return_scores=return_sequence_scores, token_scores=bool(return_token_scores),
                               share_prefix=share_prefix)
        group = n_ret if shares_prefix(self.llm_engine, share_prefix, x.shape[0] * n_ret, n_ret) else 1
        if n_ret > 1 and group == 1:
            x = x.repeat_interleave(n_ret, dim=0)                   # after the encoders and connectors, which ran once per clip
        return token_loop(self.llm_engine, x, eos, pad, max_new_tokens, processors, sample=sample, token_scores=bool(return_token_scores),
                          group=group)
