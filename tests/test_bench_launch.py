"""bench.py's rank-count contract on the CPU (no GPU call is reached): a launcher's WORLD_SIZE that differs from
--gpus, and --comm rccl with fewer GPUs than ranks, exit non-zero before anything is measured,
so a multi-GPU run can never print a line for the wrong N."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = ["--steps", "1", "--warmup", "0", "--other", "0", "--cpu-runs", "0", "--cpu-seconds", "0", "--frontend", "0",
         "--solve-all", "0", "--model-scaling", "0", "--weak", "0"]


def _run(args, **env):
    e = dict(os.environ, **env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + QUICK, cwd=ROOT, env=e,
                          capture_output=True, text=True, timeout=120)


def test_world_size_mismatch_exits_nonzero():
    r = _run(["--gpus", "1"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0 and "WORLD_SIZE=2 but --gpus 1" in r.stderr
    assert r.stdout.strip() == ""


def test_rccl_needs_one_gpu_per_rank():
    # under a launcher (WORLD_SIZE set) on a box with fewer GPUs than ranks: refused before any rendezvous (64 ranks:
    # more GPUs than any box has, so the refusal does not depend on how HIP reads an empty HIP_VISIBLE_DEVICES)
    r = _run(["--gpus", "64", "--comm", "rccl"], WORLD_SIZE="64", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0 and "one GPU per rank" in r.stderr
    assert r.stdout.strip() == ""


def _parse(monkeypatch, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


EXTRAS = ("other", "cpu_runs", "cpu_seconds", "sweep_obs", "frontend", "solve_all", "model_scaling", "weak")


def test_plain_run_measures_the_headline_alone(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full and a.steps == 7 and a.warmup == 3 and a.dump_outputs is None
    assert all(not getattr(a, k) for k in EXTRAS)


def test_full_keeps_every_measurement_and_its_switch(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3", "--full"])
    assert a.full and all(getattr(a, k) for k in EXTRAS)
    a = _parse(monkeypatch, ["--full", "--frontend", "0", "--dump-outputs", "d"])
    assert a.full and a.frontend == 0 and a.other == 1 and a.dump_outputs == "d"
    a = _parse(monkeypatch, ["--only", "sweep"])   # a profiling run of one of --full's workloads
    assert a.full and a.sweep_obs > 0 and not a.other and not a.frontend
