"""CPU check of the load planner (csrc/ba_plan.cpp: the device order, the sweep and Schur work lists, the reduce
lists, the Cholesky envelope and the Cholesky kernel choice).  tests/native/ba_plan_check.cpp plans generated
sliding-window problems and recomputes by brute force what the kernels' comments promise about the lists; the
planner and the check are built into one stand-alone program under AddressSanitizer and UBSan.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_lists_keep_the_kernels_invariants(tmp_path):
    exe = tmp_path / "ba_plan_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "ba_plan.cpp"),
                    os.path.join(ROOT, "tests", "native", "ba_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ba_plan_check OK" in out.stdout
