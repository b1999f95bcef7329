"""bench.py on the GPU: a plain run prints the headline line only and --dump-outputs writes what the last timed step computed,
the same arrays on every run with the same arguments (seeded inputs, weights and DropPath draws)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, env=env, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_steps_joints(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        j = _bench(["--config", "0", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)])
        assert j["metric"] == "frames/sec" and j["unit"] == "frames/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
        assert j["steps"] == 3 and j["ms_per_step"] > 0 and abs(j["value"] - 1 * 1e3 / j["ms_per_step"]) < 0.01 * j["value"]
        assert not {"roofline", "cpu_baseline", "vs_fp32_oracle", "sustained", "overlapped_steps", "fp32_pipe_plan"} & set(j)
        assert sorted(os.listdir(d)) == ["joints.npy"]
        runs.append(np.load(d / "joints.npy"))
    assert runs[0].dtype == np.float32 and runs[0].shape == (1, 1, 17, 3) and np.isfinite(runs[0]).all()
    assert np.array_equal(runs[0], runs[1])


def test_training_dump_is_reproducible(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        j = _bench(["--train", "--batch", "8", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)])
        assert j["steps"] == 2 and "train_phases" not in j
        runs.append({k: np.load(d / (k + ".npy")) for k in ("joints", "loss", "lifter_params_sample")})
    a, b = runs
    assert a["joints"].shape == (8, 1, 17, 3) and a["loss"].size == 1 and a["lifter_params_sample"].shape == (1 << 22,)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all()
        assert np.array_equal(a[k], b[k]), k
