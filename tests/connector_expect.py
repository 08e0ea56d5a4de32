"""Expected values for the connector-training tests, made on the CPU from the EXISTING oracle functions (nothing under oracle/ changes): autograd
through oracle.prepare_llm_inputs -> llama_hidden -> causal_lm_loss with the four connector tensors (and the LoRA tensors) as leaves.  Also
yields d loss / d inputs_embeds, what avllm_llama_lora_bwd_layers_dx leaves in dx_embeds."""
import torch

from oracle import avsr_oracle as O

CONNECTOR_KEYS = ("audio_connector.linear.weight", "audio_connector.linear.bias", "video_connector.linear.weight", "video_connector.linear.bias")


def connector_step(W, cfg, audio, video, prompt, labels, masks=None):
    """-> (loss, dx_embeds [B,S,d], {connector key: grad}, {lora key: grad}) of one training forward + backward."""
    Wc = dict(W)
    for name in ("audio_connector", "video_connector"):
        Wc[name] = {k: v.clone().requires_grad_(True) for k, v in W[name].items()}
    lora = {k: v.clone().requires_grad_(True) for k, v in W["lora"].items()}
    x, _, lab = O.prepare_llm_inputs(Wc, cfg, audio, video, prompt, labels, training=True)
    x.retain_grad()
    h = O.llama_hidden(W["llama"], lora, cfg.llama, cfg.lora, x, masks=masks)
    loss = O.causal_lm_loss(h @ W["llama"]["lm_head.weight"].T, lab)
    loss.backward()
    grads = {}
    for name in ("audio_connector", "video_connector"):
        for k, v in Wc[name].items():
            grads[f"{name}.{k}"] = v.grad if v.grad is not None else torch.zeros_like(v)
    return loss.detach(), x.grad, grads, {k: v.grad for k, v in lora.items()}
