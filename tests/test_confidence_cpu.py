"""avllm.confidence.word_confidences on hand-made cases (byte tokenizer and a sentencepiece-style stub), and the argument rules of
scripts/clip_whisper/decode.py --nbest / --confidence, which hold before any model is built."""
import math
import os
import sys

import pytest
import torch

from avllm.confidence import word_confidences
from avllm.tokenizer import ByteTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class PieceTokenizer:
    """Sentencepiece-style stub: ids index PIECES; 0 pad, 1 bos, 2 eos."""
    PIECES = ["<pad>", "<s>", "</s>", "▁the", "▁qu", "ick", "▁fox", "es", "▁a"]
    pad_token_id, bos_token_id, eos_token_id = 0, 1, 2
    all_special_ids = [0, 1, 2]

    def convert_ids_to_tokens(self, ids):
        return [self.PIECES[i] for i in ids]


def approx(got, want):
    assert [w for w, _ in got] == [w for w, _ in want], (got, want)
    for (_, a), (_, b) in zip(got, want):
        assert a == pytest.approx(b, rel=1e-12), (got, want)


def test_pieces_group_into_words():
    tok = PieceTokenizer()
    #        <s>  the   qu   ick   fox   es   </s> <pad>
    ids = [[1, 3, 4, 5, 6, 7, 2, 0]]
    lps = [[-9.0, -0.1, -0.2, -0.7, -0.3, -0.05, -0.01, -5.0]]
    approx(word_confidences(tok, ids, lps)[0], [("the", math.exp(-0.1)), ("quick", math.exp(-0.7)), ("foxes", math.exp(-0.3))])
    approx(word_confidences(tok, ids, lps, reduce="mean")[0], [("the", math.exp(-0.1)), ("quick", math.exp(-0.45)), ("foxes", math.exp(-0.175))])
    approx(word_confidences(tok, ids, lps, reduce="sum")[0], [("the", math.exp(-0.1)), ("quick", math.exp(-0.9)), ("foxes", math.exp(-0.35))])
    # tensors in, and a first token without the marker still starts a word
    out = word_confidences(tok, torch.tensor([[5, 8, 2, 0], [2, 0, 0, 0]]), torch.tensor([[-1.0, -2.0, -0.5, 0.0], [-0.5, 0.0, 0.0, 0.0]]))
    approx(out[0], [("ick", math.exp(-1.0)), ("a", math.exp(-2.0))])
    assert out[1] == []                                                  # the empty hypothesis


def test_byte_tokenizer_words():
    tok = ByteTokenizer(512)
    text = "hi yo  é"
    ids = tok.encode(text, add_bos=True) + [tok.eos_token_id, tok.pad_token_id, tok.pad_token_id]
    n = len(text.encode("utf-8"))
    lps = [-7.0] + [-0.1 * (i + 1) for i in range(n)] + [-0.3, 0.0, 0.0]
    # bytes: h i _ y o _ _ 0xc3 0xa9 -> "hi", " yo", " " (dropped), " é" (two bytes, one character)
    got = word_confidences(tok, [ids], [lps])[0]
    approx(got, [("hi", math.exp(-0.2)), ("yo", math.exp(-0.5)), ("é", math.exp(-0.9))])
    approx(word_confidences(tok, [ids], [lps], reduce="sum")[0],
           [("hi", math.exp(-0.3)), ("yo", math.exp(-1.2)), ("é", math.exp(-2.4))])
    assert " ".join(w for w, _ in got).split() == text.split()
    assert word_confidences(tok, [[tok.eos_token_id, 2, 2]], [[-0.2, 0.0, 0.0]]) == [[]]
    assert word_confidences(tok, [], []) == []


def test_bad_arguments():
    tok = ByteTokenizer(512)
    with pytest.raises(ValueError):
        word_confidences(tok, [[5]], [[-1.0]], reduce="max")
    with pytest.raises(ValueError):
        word_confidences(tok, [[5, 6]], [[-1.0]])
    with pytest.raises(ValueError):
        word_confidences(tok, [[5], [6]], [[-1.0]])


def test_decode_script_argument_rules(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts", "clip_whisper"))
    try:
        import decode
    finally:
        sys.path.pop(0)
    for argv in (["--nbest", "3", "--num_beams", "2"], ["--nbest", "0"], ["--nbest", "2", "--num_beams", "4", "--do_sample"], ["--nbest", "2"]):
        with pytest.raises(SystemExit) as e:
            decode.parse_args(argv)
        assert e.value.code == 2
    assert "--nbest" in capsys.readouterr().err
    a = decode.parse_args(["--confidence"])
    assert a.confidence and a.nbest == 1 and a.num_beams == 1 and a.min_avg_logprob is None
    a = decode.parse_args(["--nbest", "3", "--num_beams", "4", "--min_avg_logprob", "-1.5"])
    assert a.nbest == 3 and not a.confidence and a.min_avg_logprob == -1.5
    a = decode.parse_args([])
    assert a.nbest == 1 and not a.confidence
