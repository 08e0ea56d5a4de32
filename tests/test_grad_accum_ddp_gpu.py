"""GPU: grad_accum_steps = 2 under torch.distributed with 2 ranks on one card (gloo, as tests/test_connector_ddp_gpu.py): 2 ranks x 2 micro-batches
of 1 clip must equal ONE process stepping on the batch of 4, the replicas must hold the same bits, and a micro-step that does not close the
window issues no collective."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from test_connector_ddp_gpu import _build  # noqa: E402


def _build_accum(dev):
    m, _, audio, video, labels, prompt = _build(dev)
    from avllm.trainer import ClipWhisperTrainer
    tr = ClipWhisperTrainer(m, learning_rate=1e-3, grad_clip=0.5, total_steps=10, max_epochs=1, grad_accum_steps=2)
    return m, tr, audio, video, labels, prompt


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    calls, real = [0], dist.all_reduce

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)
    dist.all_reduce = counted
    m, tr, audio, video, labels, prompt = _build_accum("cuda:0")
    assert tr.reducer.enabled
    losses, after_micro0 = [], []
    for _ in range(2):
        for j in range(2):
            sl = slice(rank * 2 + j, rank * 2 + j + 1)
            before = calls[0]
            tr.train_step(audio[sl].cuda(), video[sl].cuda(), labels[sl].cuda(), prompt[sl].cuda())
            if j == 0:
                after_micro0.append(calls[0] - before)
        losses.append(float(tr.window_loss))
    torch.cuda.synchronize()
    q.put((rank, losses, after_micro0, calls[0], m.llm_engine.lora_p.cpu().numpy(), m.conn_p.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_two_micro_batches_equal_one_process(dev):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37700 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=600), q.get(timeout=600)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, losses, quiet0, n0, lora0, conn0), (_, losses1, quiet1, n1, lora1, conn1) = got
    assert quiet0 == [0, 0] and quiet1 == [0, 0], "a micro-step that does not close the window issued a collective"
    assert n0 == n1 and n0 > 0
    assert losses == losses1 and (lora0 == lora1).all() and (conn0 == conn1).all()          # replicas: the same bits
    m, tr, audio, video, labels, prompt = _build("cuda:0")
    ref_losses = [float(tr.train_step(audio.cuda(), video.cuda(), labels.cuda(), prompt.cuda())) for _ in range(2)]
    assert max(abs(a - b) for a, b in zip(losses, ref_losses)) < 2e-4, (losses, ref_losses)
    init = _build("cuda:0")[0]
    for have, ref, start in ((lora0, m.llm_engine.lora_p.cpu(), init.llm_engine.lora_p.cpu()), (conn0, m.conn_p.cpu(), init.conn_p.cpu())):
        assert float((ref - start).norm()) > 0
        rel = ((torch.from_numpy(have) - ref).norm() / (ref - start).norm()).item()
        assert rel < 2e-2, rel                                   # relative to the size of the 2-step update
