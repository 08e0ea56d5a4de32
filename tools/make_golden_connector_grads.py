#!/usr/bin/env python3
"""Write tests/golden/g11_connector_grads.npz from the REFERENCE: the loss and the four connector gradients of its training step with
freeze_encoders=False on the g2 tiny model and batch (oracle/make_golden.py golden_e2e: seed 0, batch seed 1234, B = 2, 7 frames, 50-token
prompt).  The connector gradient does not depend on whether the encoders receive one too, so these are the values train_connectors=True must
produce with the encoders frozen.  On that batch every scored label sits in the first few positions, which under causal attention and the
544 -> 256 pooling see prompt rows only: the reference's connector gradients there are exactly zero.  The file records that as max |g| per tensor ("max_abs_grad.*") and carries a second case on the
same model and inputs with the labels cut to their first 24 columns (544 -> 24 pooling: every scored position sees fused rows), keys "b.*".
Needs the reference checkout (build container only); writes data, nothing else."""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import weights as Wt  # noqa: E402
from oracle.make_golden import build_reference_model, load_reference  # noqa: E402


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    cw = load_reference()
    cfg = Wt.tiny()
    W = Wt.all_weights(cfg, 0, lora_b_std=0.05)
    audio, video, labels, _ = Wt.synthetic_batch(cfg, 2, 7, seed=1234)
    prompt = torch.randint(3, cfg.llama.vocab, (2, 50), generator=torch.Generator().manual_seed(99))
    out = {"seed": np.int64(0), "batch_seed": np.int64(1234), "frames": np.int64(7), "prompt": prompt.numpy(), "b.label_cols": np.int64(24)}
    for pre, lab in (("", labels), ("b.", labels[:, :24].contiguous())):
        m = build_reference_model(cw, cfg, W, freeze_encoders=False)
        m.train()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = m(audio=audio, video=video, prompt=prompt, labels=lab)
            res["loss"].backward()
        out[pre + "loss"] = res["loss"].detach().numpy()
        print(f"case {pre or 'g2'}: loss {float(res['loss'].detach()):.6f}")
        for name, conn in (("audio_connector", m.audio_connector), ("video_connector", m.video_connector)):
            for pn, p in conn.named_parameters():
                assert p.grad is not None, (name, pn)
                if pre:
                    out[f"{pre}grad.{name}.{pn}"] = p.grad.numpy().copy()
                else:      # exactly zero on this batch: the finding is one number per tensor, not a dense tensor of zeros
                    out[f"max_abs_grad.{name}.{pn}"] = np.float32(p.grad.abs().max())
                print(f"  {name}.{pn}: {tuple(p.grad.shape)} max |g| {float(p.grad.abs().max()):.3e}")
    path = os.path.join(ROOT, "tests", "golden", "g11_connector_grads.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
