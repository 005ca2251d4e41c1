"""CPU check of the structure-only planner (csrc/points_plan.cpp: the per-point observation ranges, the 24-byte
records, the frame table and the DID_NOT_RUN decisions that k_point_lm reads).  tests/native/points_plan_check.cpp
plans generated maps and recomputes the lists by brute force; the planner and the check are built into one
stand-alone program under AddressSanitizer and UBSan.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_points_planner_matches_brute_force(tmp_path):
    exe = tmp_path / "points_plan_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "points_plan.cpp"),
                    os.path.join(ROOT, "tests", "native", "points_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "points_plan_check OK" in out.stdout
