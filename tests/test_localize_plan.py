"""CPU check of what localization adds to the pose planner (csrc/pose_plan.cpp): the run rule kLocalizeMinObs = 4 and
each record's observation index, which sg_slam_localize_frames uses to scatter the inlier flags.
tests/native/localize_plan_check.cpp plans generated maps both ways and recomputes the lists by brute force; the
planner and the check are built into one stand-alone program under AddressSanitizer and UBSan.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_localize_planner_matches_brute_force(tmp_path):
    exe = tmp_path / "localize_plan_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "pose_plan.cpp"),
                    os.path.join(ROOT, "tests", "native", "localize_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "localize_plan_check OK" in out.stdout
