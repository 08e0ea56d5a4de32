"""The CPU reference of ClipWhisperModel.generate() that the test_generate_*_gpu.py files share: a restatement of transformers'
GenerationMixin._beam_search (`hf_beam_search`) and of its greedy / sampled loop (`token_loop`), both driving the oracle's llama_hidden
(`oracle_step_fn`) and both taking the logits processors as a function `process(scores, hist)` (a closure over
test_logits_process_cpu.restate or logits_bias_ref.chain; None = identity), and the small helpers around them."""
import numpy as np
import torch

from oracle import avsr_oracle as O
from sample_ref import kept


def trim(row, eos, pad):
    """A returned row without its padding: up to and including the first eos."""
    row = [int(t) for t in row]
    if eos is not None and eos in row:
        return row[:row.index(eos) + 1]
    return row


def h32(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def draw(probs, seed, row, step):
    """The sampling kernel's draw (csrc/sample.hip): u = 24-bit hash of (seed + row, step), inverse CDF over the kept tokens in
    vocabulary-index order.  Returns (token, distance of u to the nearer end of the token's CDF interval)."""
    u = (h32(h32((seed + row + 0x9E3779B9) & 0xFFFFFFFF) ^ step) >> 8) * 2.0 ** -24
    cum = np.cumsum(probs)
    tok = int(np.argmax(cum > u * cum[-1]))
    lo = cum[tok] - probs[tok]
    return tok, min(u * cum[-1] - lo, cum[tok] - u * cum[-1])


def edge(sorted_scores, j):
    """The gap between the j-th and the j+1-th of each row's descending scores, where the j-th is a real score (not a -1e9 placeholder)."""
    a, b = sorted_scores[:, j - 1], sorted_scores[:, j]
    live = a > -1e8
    return float((a - b)[live].min()) if bool(live.any()) else float("inf")


def token_loop(step, B, n_new, eos, pad, process, sample=None):
    """generate()'s greedy / sampled loop on the oracle's logits with the processors process(scores, hist) (None: none).
    sample = (temperature, top_k, top_p, seed) or None.  Returns (tokens [B, L], the smallest decision margin of an unfinished row)."""
    logits = step(None, None)
    hist = torch.zeros(B, 0, dtype=torch.int64)
    unfinished = torch.ones(B, dtype=torch.bool)
    margin = float("inf")
    for cur in range(n_new):
        s = logits.float() if process is None else process(logits.float(), hist)
        nxt = torch.full((B,), pad, dtype=torch.int64)
        for b in range(B):
            if not unfinished[b]:
                continue
            if sample is None:
                top = torch.topk(s[b], 2).values
                nxt[b], mg = int(torch.argmax(s[b])), float(top[0] - top[1])
            else:
                t, k, tp, seed = sample
                _, probs = kept(s[b].numpy(), t, k, tp)
                tok, mg = draw(probs, seed, b, cur)
                nxt[b] = tok
            margin = min(margin, mg)
        if eos is not None:
            unfinished = unfinished & (nxt != eos)
        hist = torch.cat([hist, nxt[:, None]], 1)
        if cur + 1 == n_new or not bool(unfinished.any()):
            break
        logits = step(nxt, torch.arange(B))
    return hist, margin


def hf_beam_search(step, B, nb, V, max_new, eos, pad, process=None, length_penalty=1.0, early_stopping=False):
    """GenerationMixin._beam_search for inputs_embeds (decoder_prompt_len = 0, max_length = max_new), one EOS id or none.
    step(tokens, beam_idx): tokens None -> the prefill logits [B*nb, V] (beams of an item repeated); otherwise reorder the cache rows by
    beam_idx [B*nb] and run one token per row.  process(log_probs, hist), None = identity, sits at _beam_search's processor call:
    log_softmax, then the processors on the log-probabilities with running_sequences[:, :, :cur_len] as their input_ids, then the running
    beam scores.  Returns (sequences [B, L], sequences_scores [B], gap): gap is the smallest gap at a selection edge of any step: between the
    k-th and k+1-th candidate, between the last running beam kept and the first dropped, and between the last finished hypothesis kept
    and the first dropped.  (The order inside a selected set only permutes the beams.)"""
    k = 2 * nb
    running_sequences = torch.full((B, nb, max_new), pad, dtype=torch.int64)
    sequences = running_sequences.clone()
    running_beam_scores = torch.zeros((B, nb))
    running_beam_scores[:, 1:] = -1e9
    beam_scores = torch.full((B, nb), -1e9)
    is_sent_finished = torch.zeros((B, nb), dtype=torch.bool)
    unsatisfied = torch.ones((B, 1), dtype=torch.bool)
    running_beam_indices = torch.full((B, nb, max_new), -1, dtype=torch.int32)
    beam_indices = running_beam_indices.clone()
    top_num_beam_mask = torch.cat((torch.ones(nb, dtype=torch.bool), torch.zeros(k - nb, dtype=torch.bool)))
    gather = lambda t, idx: torch.take_along_dim(t, idx.view(*idx.shape, *([1] * (t.dim() - 2))), dim=1)  # noqa: E731
    logits = step(None, None)
    cur_len = 0
    gap = float("inf")
    while True:
        log_probs = torch.log_softmax(logits.float(), dim=-1)
        if process is not None:
            log_probs = process(log_probs, running_sequences[:, :, :cur_len].reshape(B * nb, cur_len))
        log_probs = log_probs.view(B, nb, V) + running_beam_scores[:, :, None]
        log_probs = log_probs.reshape(B, nb * V)
        # _get_top_k_continuations
        gap = min(gap, edge(torch.topk(log_probs, k=k + 1)[0], k))                                  # which candidates make the k best
        topk_log_probs, topk_indices = torch.topk(log_probs, k=k)
        topk_beam = topk_indices // V
        topk_running_beam_indices = gather(running_beam_indices, topk_beam).clone()
        topk_running_sequences = gather(running_sequences, topk_beam).clone()
        topk_ids = topk_indices % V
        topk_running_sequences[:, :, cur_len] = topk_ids
        topk_running_beam_indices[:, :, cur_len] = (topk_beam + torch.arange(B)[:, None] * nb).to(torch.int32)
        # stopping criteria: MaxLengthCriteria, EosTokenCriteria
        hits = torch.full((B, k), cur_len + 1 >= max_new)
        if eos is not None:
            hits = hits | (topk_ids == eos)
        # _get_running_beams_for_next_iteration
        topk_running_log_probs = topk_log_probs + hits.to(torch.float32) * -1.0e9
        nxt = torch.topk(topk_running_log_probs, k=nb)[1]
        gap = min(gap, edge(torch.sort(topk_running_log_probs, dim=1, descending=True)[0], nb))     # which of them stay running beams
        running_sequences = gather(topk_running_sequences, nxt)
        running_beam_scores = gather(topk_running_log_probs, nxt)
        running_beam_indices = gather(topk_running_beam_indices, nxt)
        # _update_finished_beams
        just = hits & top_num_beam_mask[None, :]
        fin = topk_log_probs / ((cur_len + 1) ** length_penalty)
        fin += (torch.all(is_sent_finished, dim=-1, keepdim=True) & (early_stopping is True)).to(torch.float32) * -1.0e9
        fin += (~unsatisfied).to(torch.float32) * -1.0e9
        fin += (~just) * -1.0e9
        merged = torch.cat((beam_scores, fin), dim=1)
        sel = torch.topk(merged, k=nb)[1]
        gap = min(gap, edge(torch.sort(merged, dim=1, descending=True)[0], nb))                     # which hypotheses stay finished ones
        sequences = gather(torch.cat((sequences, topk_running_sequences), dim=1), sel)
        beam_scores = gather(merged, sel)
        beam_indices = gather(torch.cat((beam_indices, topk_running_beam_indices), dim=1), sel)
        is_sent_finished = gather(torch.cat((is_sent_finished, just), dim=1), sel)
        beam_idx = running_beam_indices[:, :, cur_len].reshape(-1).long()
        cur_len += 1
        # _check_early_stop_heuristic, _beam_search_has_unfinished_sequences
        best_len = max_new if (early_stopping == "never" and length_penalty > 0.0) else cur_len
        best_running = running_beam_scores[:, :1] / (best_len ** length_penalty)
        worst_finished = torch.where(is_sent_finished, torch.min(beam_scores, dim=1, keepdim=True)[0], -1.0e9)
        unsatisfied = unsatisfied & torch.any(best_running > worst_finished, dim=-1, keepdim=True)
        going = bool(torch.any(unsatisfied) & ~(torch.all(is_sent_finished) & (early_stopping is True)) & ~torch.all(hits))
        if not going:
            break
        logits = step(running_sequences[:, :, cur_len - 1].reshape(-1), beam_idx)
    L = int(((beam_indices[:, 0] + 1) != 0).sum(dim=1).max())
    return sequences[:, 0, :L], beam_scores[:, 0], gap


def oracle_step_fn(W, cfg, x, nb, lora=True):
    """The oracle's llama_hidden with a per-layer KV cache (HF's DynamicCache), reordered in full by beam_idx at every step."""
    sd, c = W["llama"], cfg.llama
    lw = W.get("lora") if lora else None
    past = [None] * c.layers
    state = {"pos": x.shape[1]}

    def step(tokens, beam_idx):
        with torch.no_grad():
            if tokens is None:
                h = O.llama_hidden(sd, lw, c, cfg.lora, x.repeat_interleave(nb, dim=0), past=past, pos0=0)
            else:
                for i in range(c.layers):
                    past[i] = (past[i][0].index_select(0, beam_idx), past[i][1].index_select(0, beam_idx))
                h = O.llama_hidden(sd, lw, c, cfg.lora, sd["model.embed_tokens.weight"][tokens][:, None], past=past, pos0=state["pos"])
                state["pos"] += 1
            return h[:, -1] @ sd["lm_head.weight"].T
    return step


def gen(m, audio, video, dev, max_new_tokens, **kw):
    """m.generate() on the batch moved to the device; the result back on the CPU.  The test files bind their own default max_new_tokens."""
    out = m.generate(audio=audio.to(dev), video=video.to(dev), max_new_tokens=max_new_tokens, **kw)
    return tuple(t.cpu() for t in out) if isinstance(out, tuple) else out.cpu()


def with_eos(m, eos):
    class _Ctx:
        def __enter__(self_):
            self_.old = m.eos_token_id
            m.eos_token_id = eos

        def __exit__(self_, *a):
            m.eos_token_id = self_.old
    return _Ctx()
