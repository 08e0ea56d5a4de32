"""Expected values for the label-smoothing / z-loss tests of the tiny golden model, made on the CPU: tests/connector_expect.connector_step with
only the loss swapped -- autograd through oracle.prepare_llm_inputs -> oracle.llama_hidden -> lm_head -> the rule of include/avllm.h
(avllm_ce_smooth_fwd), with the four connector tensors and the LoRA tensors as leaves.  At (0, 0) the rule is oracle.causal_lm_loss."""
import torch

from oracle import avsr_oracle as O


def smooth_lm_loss(logits, labels, eps, z):
    """-> (objective, nll), token means over the scored rows, in fp32 as oracle.causal_lm_loss: labels shifted by one, -100 and the last
    position unscored.  F.cross_entropy's own label_smoothing is the eps part (tests/test_loss_refs_cpu.py holds the rule to it)."""
    B, T, V = logits.shape
    shift = torch.cat([labels[:, 1:], torch.full((B, 1), -100, dtype=labels.dtype)], dim=1).reshape(-1)
    x = logits.float().view(-1, V)
    keep = shift != -100
    rows, tgt = x[keep], shift[keep]
    lse = torch.logsumexp(rows, -1)
    nll = lse - rows.gather(-1, tgt[:, None])[:, 0]
    u = lse - rows.mean(-1)
    per_row = (1.0 - eps) * nll + eps * u + z * lse * lse
    return per_row.mean(), nll.mean().detach()


def smooth_step(W, cfg, audio, video, prompt, labels, eps, z, masks=None):
    """-> (loss, nll, {connector key: grad}, {lora key: grad}) of one training forward + backward under the smoothed objective."""
    Wc = dict(W)
    for name in ("audio_connector", "video_connector"):
        Wc[name] = {k: v.clone().requires_grad_(True) for k, v in W[name].items()}
    lora = {k: v.clone().requires_grad_(True) for k, v in W["lora"].items()}
    x, _, lab = O.prepare_llm_inputs(Wc, cfg, audio, video, prompt, labels, training=True)
    h = O.llama_hidden(W["llama"], lora, cfg.llama, cfg.lora, x, masks=masks)
    loss, nll = smooth_lm_loss(h @ W["llama"]["lm_head.weight"].T, lab, eps, z)
    loss.backward()
    grads = {}
    for name in ("audio_connector", "video_connector"):
        for k, v in Wc[name].items():
            grads[f"{name}.{k}"] = v.grad if v.grad is not None else torch.zeros_like(v)
    return loss.detach(), nll, grads, {k: v.grad for k, v in lora.items()}
