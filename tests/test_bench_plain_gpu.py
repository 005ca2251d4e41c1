"""A plain bench.py run on the device: the headline line alone, and --dump-outputs' files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "local-BA iters/sec (50 KF, 20k pts)" and line["unit"] == "iters/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64" and line["n_gpus"] == 1
    assert line["steps"] == 3 and line["warmup"] == 1 and line["solver"]["nranks"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-12)
    # nothing but the headline was measured
    for k in ("lm_regime", "solve_from_start", "roofline", "roofline_sweep", "roofline_sweep_scaled",
              "solve_all_frames", "kernel_ms_per_iter", "cpu_baseline", "strong_scaling_model", "other_workload",
              "frontend"):
        assert line[k] is None, k
    cfg = line["config"]
    shapes = {"q": (cfg["keyframes"], 4), "t": (cfg["keyframes"], 3), "X": (cfg["landmarks"], 4), "cost": (1,)}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in shapes)
    got = {n: np.load(out / (n + ".npy")) for n in shapes}
    for n, a in got.items():
        assert a.dtype == np.float64 and a.shape == shapes[n] and np.isfinite(a).all(), n
    assert sum(a.nbytes for a in got.values()) <= 64e6
    # unit quaternions, and the cost the line reports for the same state
    assert np.abs(np.linalg.norm(got["q"], axis=1) - 1.0).max() < 1e-12
    assert got["cost"][0] == line["lm_state"]["final_cost"]
