"""Expected values for the connector-training tests, made on the CPU from the EXISTING oracle functions (nothing under oracle/ changes): autograd
through oracle.prepare_llm_inputs -> llama_hidden -> causal_lm_loss with the four connector tensors (and the LoRA tensors) as leaves.  Also
yields d loss / d inputs_embeds, what avllm_llama_lora_bwd_layers_dx leaves in dx_embeds.

modes (one per clip: 0 both, 1 audio only, 2 video only) replaces the fusion of oracle.encode by tests/refs64_modality.fuse_pool_rows, which also
pools / interpolates to the label width; everything before it (the encoders, the connectors) and after it (the LLM, the loss) is the oracle's.
dtype=torch.float64 runs what the oracle's functions run in the dtype of their inputs in float64: the connectors, the fusion, the LLM layers
and lm_head.  Two parts do not take the dtype of their inputs and stay fp32: the encoders (oracle.encode calls them on `.float()` inputs, and
they are frozen: no gradient passes through them) and the cross entropy (causal_lm_loss casts the logits with `.float()`).
With the default arguments the function is the one it was, bit for bit (tests/test_trainer_cases_cpu.py asserts it)."""
import torch

from oracle import avsr_oracle as O

CONNECTOR_KEYS = ("audio_connector.linear.weight", "audio_connector.linear.bias", "video_connector.linear.weight", "video_connector.linear.bias")


def _inputs_with_modes(Wc, W, cfg, audio, video, prompt, labels, modes, dtype, wrong=()):
    """prepare_llm_inputs(training=True) with a mode per clip: the same encoders and connectors, refs64_modality's fusion and pooling.
    wrong "dropped_stream_grad": the forward is the right one, the backward also hands the pooled gradient to the stream a clip dropped."""
    import refs64_modality as RM
    with torch.no_grad():
        ha = O.whisper_encoder(W["whisper"], cfg.whisper, audio.float())
        B, Fr = video.shape[:2]
        hv = O.clip_vision_cls(W["clip"], cfg.clip, video.float().reshape(B * Fr, 3, video.shape[3], video.shape[4])).view(B, Fr, -1)
    a = O.connector(Wc["audio_connector"], ha.to(dtype))
    v = O.connector(Wc["video_connector"], hv.to(dtype))
    L = min(cfg.max_seq_len, max(a.shape[1], v.shape[1]))
    pe = None if prompt is None else W["llama"]["model.embed_tokens.weight"][prompt[:, : cfg.max_prompt_len]].to(dtype)
    lab = labels.clone()
    lab[lab == cfg.pad_token_id] = -100
    modes = [int(m) for m in modes]
    x = RM.fuse_pool_rows(a, v, pe, modes, L, lab.shape[1], cfg.fusion_scale, dtype=dtype)
    if "dropped_stream_grad" in wrong:
        other = [RM.AUDIO if m == RM.VIDEO else RM.VIDEO if m == RM.AUDIO else RM.BOTH for m in modes]
        sel = torch.tensor([0.0 if m == RM.BOTH else 1.0 for m in other], dtype=dtype).view(-1, 1, 1)
        extra = RM.fuse_pool_rows(a * sel, v * sel, None if pe is None else torch.zeros_like(pe), other, L, lab.shape[1], cfg.fusion_scale, dtype=dtype)
        x = x + (extra - extra.detach())
    return x, lab


def connector_step(W, cfg, audio, video, prompt, labels, masks=None, modes=None, dtype=None, wrong=()):
    """-> (loss, dx_embeds [B,S,d], {connector key: grad}, {lora key: grad}) of one training forward + backward.  wrong: planted defects
    (tests/refs64_trainer.py), acted on only where modes are given."""
    if modes is None and dtype is None:
        Wc = dict(W)
        for name in ("audio_connector", "video_connector"):
            Wc[name] = {k: v.clone().requires_grad_(True) for k, v in W[name].items()}
        lora = {k: v.clone().requires_grad_(True) for k, v in W["lora"].items()}
        x, _, lab = O.prepare_llm_inputs(Wc, cfg, audio, video, prompt, labels, training=True)
        x.retain_grad()
        h = O.llama_hidden(W["llama"], lora, cfg.llama, cfg.lora, x, masks=masks)
        loss = O.causal_lm_loss(h @ W["llama"]["lm_head.weight"].T, lab)
    else:
        dt = torch.float32 if dtype is None else dtype
        Wc = {name: {k: v.to(dt).clone().requires_grad_(True) for k, v in W[name].items()} for name in ("audio_connector", "video_connector")}
        lora = {k: v.to(dt).clone().requires_grad_(True) for k, v in W["lora"].items()}
        llama = W["llama"] if dt == torch.float32 else _cast(W["llama"], dt)
        if modes is None:                                          # float64 without modes: every clip fuses both streams
            modes = [0] * audio.shape[0]
        x, lab = _inputs_with_modes(Wc, W, cfg, audio, video, prompt, labels, modes, dt, wrong)
        x.retain_grad()
        if masks is not None:
            masks = {k: m.to(dt) for k, m in masks.items()}
        h = O.llama_hidden(llama, lora, cfg.llama, cfg.lora, x, masks=masks)
        loss = O.causal_lm_loss(h @ llama["lm_head.weight"].T, lab)
    loss.backward()
    grads = {}
    for name in ("audio_connector", "video_connector"):
        for k, v in Wc[name].items():
            grads[f"{name}.{k}"] = v.grad if v.grad is not None else torch.zeros_like(v)
    return loss.detach(), x.grad, grads, {k: v.grad for k, v in lora.items()}


_CAST = {}


def _cast(sd, dtype):
    """A state dict in another dtype, made once per dict (the frozen LLM weights are the same object in every call of a test)."""
    key = (id(sd), dtype)
    if key not in _CAST:
        _CAST[key] = (sd, {k: v.to(dtype) for k, v in sd.items()})
    return _CAST[key][1]
