"""Decoding behind ClipWhisperModel.generate(): the argument rules (parse_arguments), the seven logits processors as one object
(LogitsProcessors), the greedy / sampled token loop (token_loop) and HF's beam search (beam_search).  The loops are plain functions of an
engine (LlamaEngine: alloc_cache, prefill, decode_step), the LLM inputs x [B, S, d] and the EOS / pad ids; the scores stay in avllm.ops."""
import math
import numbers
from typing import NamedTuple, Optional

import torch

from . import ops
from .tokenizer import phrase_token_ids


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


class LogitsProcessors:
    """HF's seven logits processors of one generate() call, in GenerationMixin._get_logits_processor's order and in one launch
    (ops.logits_process).  The device tables of the four list keywords are built here, once (ops.logits_bias_tables; its capacities are
    refused by name).  on: any of the seven is; when none is, nothing is allocated and apply() launches nothing.  reads_history: the
    three older processors, or a table entry of more than one token, read a row's generated tokens; the kernel holds at most
    LOGITS_PROCESS_MAX_HISTORY of them, so then, and only then, max_new_tokens is limited."""

    def __init__(self, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, sequence_bias=None, bad_words_ids=None,
                 suppress_tokens=None, begin_suppress_tokens=None, *, vocab, eos, device, max_new_tokens):
        older = ops.check_logits_processors(repetition_penalty, no_repeat_ngram_size, min_new_tokens)
        self.older, self.eos = (float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens)), eos
        self.tables = ops.logits_bias_tables(sequence_bias, bad_words_ids, suppress_tokens, begin_suppress_tokens, vocab=vocab, eos=eos,
                                             device=device)                     # {} when all four are None
        self.on = older or bool(self.tables)
        self.reads_history = older or any(isinstance(t, ops.SequenceTable) and t.max_len > 1 for t in self.tables.values())
        if self.reads_history and max_new_tokens > ops.LOGITS_PROCESS_MAX_HISTORY:
            raise ValueError(f"repetition_penalty / no_repeat_ngram_size / min_new_tokens, and sequence_bias / bad_words_ids with sequences of "
                             f"more than one token, support at most {ops.LOGITS_PROCESS_MAX_HISTORY} new tokens, got max_new_tokens = "
                             f"{max_new_tokens}")

    def apply(self, scores, history, cur, append=None, log_softmax=False):
        """The chain in place on scores [rows, V]; row r's first `cur` entries of history [rows, ld] are its generated tokens.  append: int64
        [rows], stored at history[:, cur - 1] first; log_softmax: the rows become log-probabilities first (beam search).  The history and
        append are handed on only when something reads them."""
        if self.on:
            hist = self.reads_history
            ops.logits_process(scores, history if hist else None, cur, *self.older, eos=self.eos, log_softmax=log_softmax,
                               append=append if hist else None, **self.tables)


def parse_arguments(tokenizer, vocab, eos, device, *, max_new_tokens, max_length, do_sample, temperature, top_k, top_p, seed, num_beams,
                    early_stopping, return_sequence_scores, repetition_penalty, no_repeat_ngram_size, min_new_tokens, sequence_bias,
                    bad_words_ids, suppress_tokens, begin_suppress_tokens, hotwords, hotword_bias, num_return_sequences, share_prefix=False):
    """generate()'s argument rules, all of them, before any GPU work but the processors' small tables: ValueError / NotImplementedError
    that name the argument and its limit.  Returns (max_new_tokens, num_return_sequences, sample, processors); sample is (temperature,
    top_k, top_p, seed) or None, and seed=None is drawn here, once, from torch's default CPU generator."""
    if max_new_tokens is None:
        max_new_tokens = max_length if max_length is not None else 100
    if not isinstance(share_prefix, bool):
        raise ValueError(f"share_prefix must be True or False, got {share_prefix!r}")
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
    if num_beams > 1 and n_ret > num_beams:
        raise ValueError(f"num_return_sequences ({n_ret}) has to be smaller or equal to num_beams ({num_beams})")
    if num_beams == 1 and not do_sample and n_ret > 1:
        raise ValueError(f"greedy decoding cannot return {n_ret} sequences: num_return_sequences > 1 needs do_sample=True or num_beams > 1")
    sample = None
    if do_sample:
        ops.check_sampling(temperature, top_k, top_p)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        sample = (temperature, top_k, top_p, seed)
    if hotwords:
        sequence_bias = hotword_sequence_bias(tokenizer, hotwords, hotword_bias, sequence_bias)
    return max_new_tokens, int(n_ret), sample, LogitsProcessors(
        repetition_penalty, no_repeat_ngram_size, min_new_tokens, sequence_bias, bad_words_ids, suppress_tokens, begin_suppress_tokens,
        vocab=vocab, eos=eos, device=device, max_new_tokens=max_new_tokens)


def shares_prefix(engine, share_prefix, rows, group):
    """Whether a decode of `rows` rows, `group` per item, runs on one prefix cache per item: asked for, something to share, and the fused
    token step (LlamaEngine.decode_shares_prefix).  Otherwise today's path, whose result is bit-equal to share_prefix=False."""
    return bool(share_prefix) and group > 1 and engine.decode_shares_prefix(rows)


def token_loop(engine, x, eos, pad, max_new_tokens, processors, sample=None, token_scores=False, group=1):
    """GenerationMixin's greedy search, or with sample = (temperature, top_k, top_p, seed) its sampling, for inputs_embeds x [B, S, d]: the
    prefill, then per token the processors, one selection step and the next decode step.  Returns the new tokens int64 [B, L], pad after a
    row's EOS, L <= max_new_tokens (the loop ends when every row has its EOS: one host sync per step, only with an EOS id); with
    token_scores a GenerateOutput: the chosen token's log-probability and its row's entropy (ops.row_scores, at the token step; no second
    prefill), 0.0 for rows that were finished before the step.
    group > 1 (sampled n-best on a shared prefix; the caller has asked shares_prefix): x holds each item ONCE, the prefill runs on its B rows
    and the B * group rows of the loop (item-major, as x.repeat_interleave(group) would order them) read the item's prefix cache and keep
    only their generated positions in a suffix cache (LlamaEngine.decode_step_shared).  Seeds, history and EOS stay per row."""
    B, S, _ = x.shape
    if group > 1:
        kc0, vc0 = engine.alloc_cache(B, S, rows=B * group)
        logits, _ = engine.prefill(x, kc0, vc0)
        logits = logits.repeat_interleave(group, dim=0)
        B *= group
        kc, vc = engine.alloc_suffix_cache(B, max_new_tokens)
    else:
        kc, vc = engine.alloc_cache(B, S + max_new_tokens)
        logits, _ = engine.prefill(x, kc, vc)
    unfinished = torch.ones(B, dtype=torch.bool, device=x.device)
    # the processors' history: row b's generated tokens (pad after its EOS, as HF feeds them); the kernel itself appends the last token
    hist = torch.full((B, max_new_tokens), pad, dtype=torch.int64, device=x.device) if processors.reads_history else None

    # One selection step per strategy -> (tokens, logprob or None, entropy or None).  Each does the sampling kernel's bookkeeping: a finished
    # row gets the pad token and logprob 0, a row that chooses EOS is turned off in `unfinished`, in place.  The entropy is not masked.
    def greedy(logits, step):                   # logprob: log-softmax of the processed logits at the argmax (HF's normalize_logits=True)
        nxt = ops.argmax_rows(logits)
        lp = ent = None
        if token_scores:
            lp, ent = ops.row_scores(logits, nxt, entropy=True)
            lp = torch.where(unfinished, lp, torch.zeros_like(lp))
        if eos is not None:
            nxt = torch.where(unfinished, nxt, torch.full_like(nxt, pad))
            unfinished.logical_and_(nxt != eos)
        return nxt, lp, ent

    def sampled(logits, step):                  # temperature -> top_k -> top_p -> one draw per row, row b with seed + b
        temperature, top_k, top_p, seed = sample
        nxt = ops.sample_rows(logits, temperature, top_k, top_p, seed, step, unfinished=unfinished if eos is not None else None, eos=eos,
                              pad=pad, row_seeds=row_seeds, return_logprob=token_scores)
        if not token_scores:
            return nxt, None, None
        # the draw's log-probability under the distribution it was drawn from; the entropy of the UNTRUNCATED distribution
        return nxt[0], nxt[1], ops.row_scores(logits, nxt[0], temperature, entropy=True)[1]

    select = sampled if sample else greedy
    row_seeds = torch.arange(B, dtype=torch.int32, device=x.device) if sample else None
    out, tok_lp, tok_ent, nxt = [], [], [], None
    for step in range(max_new_tokens):
        processors.apply(logits, hist, step, append=nxt)
        alive = unfinished.clone() if token_scores else None        # rows that still choose a token at this step
        nxt, lp, ent = select(logits, step)
        out.append(nxt)
        if token_scores:
            tok_lp.append(lp)
            tok_ent.append(torch.where(alive, ent, torch.zeros_like(ent)))
        if step + 1 == max_new_tokens or (eos is not None and not bool(unfinished.any())):
            break
        logits = engine.decode_step_shared(nxt, step, kc0, vc0, kc, vc, group) if group > 1 else engine.decode_step(nxt, S + step, kc, vc)
    seqs = torch.stack(out, dim=1)
    return GenerateOutput(seqs, None, torch.stack(tok_lp, dim=1), torch.stack(tok_ent, dim=1)) if token_scores else seqs


def beam_search(engine, x, eos, pad, max_new_tokens, nb, length_penalty, early_stopping, processors, n_ret=1, return_scores=False,
                token_scores=False, share_prefix=False):
    """GenerationMixin._beam_search (transformers 5.x, generation/utils.py) for inputs_embeds x [B, S, d]: decoder_prompt_len = 0, so a
    hypothesis of n tokens (its EOS included) is normalised by n ** length_penalty, and max_length = max_new_tokens.  Per token step:
    the B*nb-row decode step, ops.beam_topk (log_softmax + _get_top_k_continuations, k = 2*nb), HF's bookkeeping
    (_get_running_beams_for_next_iteration, _update_finished_beams, _check_early_stop_heuristic,
    _beam_search_has_unfinished_sequences) restated on small device tensors, and ops.kv_gather_rows (ops.kv8_gather_rows when the engine
    hands out fp8 cache images: LlamaEngine.alloc_cache) reordering only the generated
    positions [S, S + step): every beam of an item shares the prefix [0, S), which is copied once from the B-row prefill cache.
    Equal scores keep candidate order (stable sorts where HF calls torch.topk).  One host sync per step, for the stopping test.
    B*nb <= 16 rows take the fused bf16 token step (LlamaEngine.decode_is_fused); more rows take the general step.
    processors: HF runs its logits processors between the log_softmax and the addition of the running beam scores, on
    running_sequences[:, :, :cur]; processors.apply(log_softmax=True) does both on the B*nb rows and beam_topk then takes log-probabilities.
    Returns the n_ret best finished hypotheses of each item, rows [B*n_ret, L] item-major, best first (HF's num_return_sequences), padded
    with pad; with return_scores also HF's sequences_scores [B*n_ret]; with token_scores a GenerateOutput: every candidate's own
    log-probability, read from the row it came from (the processed log-probability with processors on; logit - logsumexp of the raw row
    otherwise, ops.row_scores), and that row's entropy ride with the sequences as payloads [B, nb, N] through every reordering.  Never
    derived as topk_lp - running_scores[parent]: that difference loses the low bits of a long hypothesis.
    share_prefix (and shares_prefix(engine, ..., B*nb, nb)): no broadcast; the B-row prefill cache stays the prefix of every beam, the R rows
    keep only their generated positions [0, N) in a suffix cache, which is what the reordering moves, and the step is
    LlamaEngine.decode_step_shared.  More than 16 rows, fp32, or the fused step switched off: the path above, bit for bit."""
    dev = x.device
    B, S, _ = x.shape
    R, k, N = B * nb, 2 * nb, max_new_tokens
    kc0, vc0 = engine.alloc_cache(B, S, rows=R)                 # in the form of the R-row cache it is broadcast into
    logits, _ = engine.prefill(x, kc0, vc0)
    share = shares_prefix(engine, share_prefix, R, nb)
    # shared: kc0 / vc0 stay the items' prefix, the R rows keep their generated positions [0, N) alone; else the prefix is broadcast into [0, S)
    # of an R-row cache whose generated positions start at g0 = S
    kc, vc = engine.alloc_suffix_cache(R, N) if share else engine.alloc_cache(R, S + N)
    g0 = 0 if share else S
    gather_rows = ops.kv8_gather_rows if kc.dtype == torch.uint8 else ops.kv_gather_rows      # fp8 images: codes and exponents together
    if not share:
        gather_rows(kc0, vc0, kc, vc, torch.arange(R, device=dev, dtype=torch.int32) // nb, 0, S)    # prefix broadcast
        del kc0, vc0
    logits = logits.repeat_interleave(nb, dim=0)                # step 0: every beam of an item sees the prefill logits
    NEG = -1.0e9
    # the per-hypothesis payloads of the running beams, and (fin) of the finished ones
    run = {"seq": torch.full((B, nb, N), pad, dtype=torch.int64, device=dev)}
    for name in ("lp", "ent") if token_scores else ():
        run[name] = torch.zeros((B, nb, N), dtype=torch.float32, device=dev)
    fin = {name: t.clone() for name, t in run.items()}
    running_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
    running_scores[:, 1:] = NEG
    beam_scores = torch.full((B, nb), NEG, dtype=torch.float32, device=dev)
    lengths = torch.zeros((B, nb), dtype=torch.int64, device=dev)             # generated length of each finished hypothesis
    is_sent_finished = torch.zeros((B, nb), dtype=torch.bool, device=dev)
    unsatisfied = torch.ones((B, 1), dtype=torch.bool, device=dev)
    top_mask = torch.arange(k, device=dev) < nb
    offset = (torch.arange(B, device=dev, dtype=torch.int32) * nb)[:, None]
    done_host = torch.zeros(1, dtype=torch.bool).pin_memory()
    ev = torch.cuda.Event()
    for cur in range(N):
        # _get_top_k_continuations
        processors.apply(logits, run["seq"].view(R, N), cur, log_softmax=True)
        topk_lp, topk_beam, topk_tok = ops.beam_topk(logits, running_scores.view(-1), nb, k, logprobs=processors.on)
        topk_parent = topk_beam + offset
        cand = {name: torch.gather(t, 1, topk_beam.long()[:, :, None].expand(B, k, N)) for name, t in run.items()}
        cand["seq"][:, :, cur] = topk_tok
        if token_scores:
            # the candidates' own log-probabilities and their rows' entropies, from the B*nb rows beam_topk selected from
            norm, row_ent = ops.row_scores(logits, None, entropy=True, logprobs=processors.on)    # norm: -logsumexp (0 for log-probabilities)
            cand_lp = logits[topk_parent.long(), topk_tok]
            if not processors.on:
                cand_lp = cand_lp + norm[topk_parent.long()]
            cand["lp"][:, :, cur] = cand_lp
            cand["ent"][:, :, cur] = row_ent[topk_parent.long()]
        # stopping criteria: EOS, or max_length reached
        last = cur + 1 >= N
        hits = topk_tok == eos if eos is not None and not last else torch.full((B, k), last, dtype=torch.bool, device=dev)
        # _get_running_beams_for_next_iteration
        topk_running_lp = topk_lp + hits.to(torch.float32) * NEG
        nxt = torch.sort(topk_running_lp, dim=1, descending=True, stable=True)[1][:, :nb]
        run = {name: torch.gather(t, 1, nxt[:, :, None].expand(B, nb, N)) for name, t in cand.items()}
        running_scores = torch.gather(topk_running_lp, 1, nxt)
        parent = torch.gather(topk_parent, 1, nxt)
        # _update_finished_beams
        just = hits & top_mask[None, :]
        fin_lp = topk_lp / ((cur + 1) ** length_penalty)
        full = torch.all(is_sent_finished, dim=-1, keepdim=True) & (early_stopping is True)
        fin_lp += full.to(torch.float32) * NEG
        fin_lp += (~unsatisfied).to(torch.float32) * NEG
        fin_lp += (~just) * NEG
        m_scores = torch.cat((beam_scores, fin_lp), dim=1)
        sel = torch.sort(m_scores, dim=1, descending=True, stable=True)[1][:, :nb]
        fin = {name: torch.gather(torch.cat((t, cand[name]), dim=1), 1, sel[:, :, None].expand(B, nb, N)) for name, t in fin.items()}
        beam_scores = torch.gather(m_scores, 1, sel)
        lengths = torch.gather(torch.cat((lengths, torch.full((B, k), cur + 1, dtype=torch.int64, device=dev)), dim=1), 1, sel)
        is_sent_finished = torch.gather(torch.cat((is_sent_finished, just), dim=1), 1, sel)
        if last:                                                # every candidate hit max_length: HF's loop ends here
            break
        # _check_early_stop_heuristic at cur_len = cur + 1, then _beam_search_has_unfinished_sequences
        best_len = N if early_stopping == "never" and length_penalty > 0.0 else cur + 1
        best_running = running_scores[:, :1] / (best_len ** length_penalty)
        worst_finished = torch.where(is_sent_finished, torch.min(beam_scores, dim=1, keepdim=True)[0], NEG)
        unsatisfied = unsatisfied & torch.any(best_running > worst_finished, dim=-1, keepdim=True)
        done = ~(torch.any(unsatisfied) & ~(torch.all(is_sent_finished) & (early_stopping is True)) & ~torch.all(hits))
        done_host.copy_(done.view(1), non_blocking=True)
        ev.record()
        # the next token step is queued before the host waits on the stopping test (only the small copy above is awaited)
        gather_rows(kc, vc, kc, vc, parent.view(-1).to(torch.int32), g0, g0 + cur)
        ids = run["seq"][:, :, cur].reshape(-1)
        logits = engine.decode_step_shared(ids, cur, kc0, vc0, kc, vc, nb) if share else engine.decode_step(ids, S + cur, kc, vc)
        ev.synchronize()
        if bool(done_host[0]):
            break
    L = int(lengths[:, :n_ret].max())
    out = {name: t[:, :n_ret, :L].reshape(B * n_ret, L) for name, t in fin.items()}
    scores = beam_scores[:, :n_ret].reshape(B * n_ret)
    if token_scores:
        return GenerateOutput(out["seq"], scores, out["lp"], out["ent"])
    return (out["seq"], scores) if return_scores else out["seq"]
