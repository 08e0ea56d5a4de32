"""bench.py's two run modes, each as a child process at the tiny size: a plain run prints the headline line and writes --dump-outputs
and runs no secondary leg; --full adds them (at the tiny size only the CPU baseline applies, taken here in its sampled form)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--gpus", "1", "--steps", "2", "--warmup", "2", "--tiny", "--batch", "2", "--frames", "3"]
SECONDARY = ("cpu_baseline", "decode", "variants")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *TINY, *extra], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_is_headline_only(dev, tmp_path):
    out = _bench("--dump-outputs", str(tmp_path))
    assert out["unit"] == "samples/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["steps"] == 2 and out["warmup"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 2 * 1000 / out["ms_per_step"]) <= 1e-3 * out["value"]          # 2 clips per step
    assert out["config"]["launch"] == "hipGraph replay" and "roofline" in out
    assert not [k for k in SECONDARY if k in out] and "host_inputs" not in out["config"]
    assert sorted(os.listdir(tmp_path)) == ["lora_grads.npy", "lora_params.npy", "loss.npy"]


@pytest.mark.gpu
def test_bench_full_run_adds_secondary_legs(dev):
    out = _bench("--full", "--cpu-baseline", "sample")
    assert out["steps"] == 2 and out["value"] > 0
    assert out["cpu_baseline"]["unit"] == "samples/s" and out["cpu_baseline"]["value"] > 0
