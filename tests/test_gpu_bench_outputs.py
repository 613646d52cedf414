"""bench.py's plain run (no --full): the headline line alone, and --dump-outputs writes what the last timed step
returned -- the last Linear's output and the logits, float32 -- with the same bits from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_bench(out_dir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_dumps_the_last_step_and_repeats_it_bit_for_bit(tmp_path):
    runs = []
    for i in range(2):
        line = _plain_bench(tmp_path / str(i))
        assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
        assert line["unit"] == "tokens/s" and line["higher_is_better"] is True and line["dtype"] == "int8"
        assert line["value"] > 0 and line["ms_per_step"] > 0
        assert abs(line["value"] - 768 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
        assert not {"roofline", "full_prefill", "cpu_baseline", "cpu_baseline_port", "secondary", "logits_check"} & set(line)
        assert sorted(os.listdir(tmp_path / str(i))) == ["last_linear_out.npy", "logits.npy"]
        y = np.load(tmp_path / str(i) / "last_linear_out.npy")
        logits = np.load(tmp_path / str(i) / "logits.npy")
        assert y.dtype == np.float32 and y.shape == (768, 3584) and np.isfinite(y).all() and np.abs(y).max() > 0
        assert logits.dtype == np.float32 and logits.shape == (1, 152064) and np.isfinite(logits).all()
        runs.append((y, logits))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
