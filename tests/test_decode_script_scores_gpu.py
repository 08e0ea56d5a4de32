"""scripts/clip_whisper/decode.py --nbest / --confidence on the tiny model: the n-best list, token log-probabilities and word confidences in
the --output_file JSON, and exactly the earlier keys without the flags."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_decode_script_nbest_and_confidence(dev, tmp_path):
    from test_data_cpu import make_set
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = tmp_path / "toy"
    data.mkdir()
    mp, lp = make_set(data, n=4)
    out = tmp_path / "out"
    # one subprocess, two decodes: the script's main() runs without and with the new flags in one interpreter
    prog = ("import sys, runpy; m = runpy.run_path(sys.argv[1], run_name='decode_script'); base = sys.argv[2:]; "
            "sys.exit(m['main'](base + ['--output_file', 'plain.json']) or m['main'](base + ['--output_file', 'scored.json', "
            "'--num_beams', '4', '--nbest', '2', '--confidence', '--min_avg_logprob', '-1.0']))")
    r = subprocess.run([sys.executable, "-c", prog, os.path.join(root, "scripts/clip_whisper/decode.py"), "--test_data", str(mp), "--test_wrd",
                        str(lp), "--output_dir", str(out), "--batch_size", "2", "--max_new_tokens", "6", "--tiny", "--data_path", str(data)],
                       capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=root), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    plain = json.load(open(out / "plain.json"))
    assert set(plain) == {"modality", "overall_wer", "total_samples", "results"} and len(plain["results"]) == 4
    for u in plain["results"]:
        assert set(u) == {"utt_id", "hypothesis", "reference", "wer"}
    scored = json.load(open(out / "scored.json"))
    assert len(scored["results"]) == 4
    for u in scored["results"]:
        assert set(u) == {"utt_id", "hypothesis", "reference", "wer", "tokens", "token_logprobs", "avg_logprob", "word_confidences", "nbest"}
        assert len(u["nbest"]) == 2 and u["nbest"][0]["hypothesis"] == u["hypothesis"] and u["nbest"][0]["score"] >= u["nbest"][1]["score"]
        assert 1 <= len(u["tokens"]) <= 6 and len(u["token_logprobs"]) == len(u["tokens"])
        assert all(v <= 0.0 for v in u["token_logprobs"]) and min(u["token_logprobs"]) < 0.0
        assert u["avg_logprob"] == pytest.approx(sum(u["token_logprobs"]) / len(u["token_logprobs"]), abs=1e-12)
        assert " ".join(w for w, _ in u["word_confidences"]).split() == u["hypothesis"].split()
        assert all(0.0 < c <= 1.0 for _, c in u["word_confidences"])
    logs = [f for f in os.listdir(out) if f.startswith("decode_") and f.endswith(".log")]
    assert any("avg_logprob < -1.0" in open(out / f).read() for f in logs)
