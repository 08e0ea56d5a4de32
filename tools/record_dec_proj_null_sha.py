#!/usr/bin/env python3
"""Print the NULL_BIAS_SHA table of tests/test_dec_proj_bias_gpu.py as a given tree's library computes it (needs the GPU):
    python tools/record_dec_proj_null_sha.py /path/to/a/built/checkout
The inputs and the checksum come from this tree's test file, the avllm package (and its libavllm.so) from the checkout named, which may be
older than the bias term: null_bias_cases passes no argument that such a library lacks.  Run it on the parent of a commit that changes
dec_proj's summation order, never on the commit itself."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tree = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else ROOT)
sys.path[:0] = [os.path.join(tree, "audio-visual-llm_amd"), ROOT, os.path.join(ROOT, "tests")]
import avllm  # noqa: E402
import test_dec_proj_bias_gpu as T  # noqa: E402

print("package:", os.path.dirname(avllm.__file__))
for form in T.FORMS:
    print(f'    "{form}": "{T.checksum(T.null_bias_cases(form)[3])}",')
