"""Word confidences from generate(return_token_scores=True): token log-probabilities grouped into words by the tokenizer's own word
boundaries.  Pure host code (lists, tensors or arrays in; Python lists out)."""
from __future__ import annotations

import math

from .tokenizer import ByteTokenizer

_WORD_START = ("▁", "Ġ", " ")             # sentencepiece's and byte-level BPE's markers of a leading space, and the space itself
_REDUCE = {"min": min, "mean": lambda v: sum(v) / len(v), "sum": sum}


def _special_ids(tokenizer):
    if isinstance(tokenizer, ByteTokenizer):
        return {tokenizer.unk_token_id, tokenizer.bos_token_id, tokenizer.eos_token_id, tokenizer.pad_token_id}
    ids = set(getattr(tokenizer, "all_special_ids", None) or [])
    for name in ("pad_token_id", "eos_token_id", "bos_token_id"):
        if getattr(tokenizer, name, None) is not None:
            ids.add(int(getattr(tokenizer, name)))
    return ids


def _pieces(tokenizer, ids):
    """One string per token whose first character tells whether the token starts a word."""
    if not isinstance(tokenizer, ByteTokenizer) and hasattr(tokenizer, "convert_ids_to_tokens"):
        return [str(p) for p in tokenizer.convert_ids_to_tokens(ids)]
    return [tokenizer.decode([i], skip_special_tokens=True) for i in ids]


def _word_text(tokenizer, ids, pieces):
    if not isinstance(tokenizer, ByteTokenizer) and hasattr(tokenizer, "convert_ids_to_tokens"):
        if hasattr(tokenizer, "convert_tokens_to_string"):
            text = tokenizer.convert_tokens_to_string(pieces)
        else:
            text = "".join(pieces).replace("▁", " ").replace("Ġ", " ")
    else:
        text = tokenizer.decode(ids, skip_special_tokens=True)     # the bytes of the whole word: a character may span several tokens
    return text.lstrip(" ")


def word_confidences(tokenizer, ids, token_logprobs, reduce="min"):
    """[(word, confidence), ...] for every utterance of ids [rows, L] with token_logprobs [rows, L] (generate()'s sequences and
    token_scores, or lists of lists).  A token starts a word when it is the first kept token of the utterance or its piece begins with a
    space: `convert_ids_to_tokens` pieces with the leading-space markers of sentencepiece / byte-level BPE where the tokenizer has them,
    the decoded text of the token for the byte tokenizer.  The confidence of a word is exp(min | mean | sum of its tokens' log-probabilities).
    A row ends at its first EOS; special and pad tokens are dropped; groups that hold nothing but spaces are dropped."""
    if reduce not in _REDUCE:
        raise ValueError(f"reduce must be one of {sorted(_REDUCE)}, got {reduce!r}")
    if hasattr(ids, "tolist"):
        ids = ids.tolist()
    if hasattr(token_logprobs, "tolist"):
        token_logprobs = token_logprobs.tolist()
    if len(ids) != len(token_logprobs):
        raise ValueError(f"{len(ids)} rows of ids but {len(token_logprobs)} rows of token_logprobs")
    special = _special_ids(tokenizer)
    eos = getattr(tokenizer, "eos_token_id", None)
    out = []
    for row, lps in zip(ids, token_logprobs):
        if len(row) != len(lps):
            raise ValueError(f"a row of {len(row)} ids has {len(lps)} token_logprobs")
        kept = []
        for t, lp in zip(row, lps):
            if eos is not None and int(t) == eos:
                break
            if int(t) not in special:
                kept.append((int(t), float(lp)))
        pieces = _pieces(tokenizer, [t for t, _ in kept])
        groups = []
        for (t, lp), piece in zip(kept, pieces):
            if not groups or piece.startswith(_WORD_START):
                groups.append(([], [], []))
            g = groups[-1]
            g[0].append(t); g[1].append(piece); g[2].append(lp)
        words = []
        for g_ids, g_pieces, g_lps in groups:
            text = _word_text(tokenizer, g_ids, g_pieces)
            if text:
                words.append((text, math.exp(_REDUCE[reduce](g_lps))))
        out.append(words)
    return out
