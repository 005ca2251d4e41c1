"""CPU check of the iteration-chain planner (csrc/ba_chain.cpp: which kernels one LM iteration launches, in which
order and mode, in every regime of knobs, ranks and Cholesky path).  tests/native/chain_plan_check.cpp compares the
named regimes with literal sequences and checks, over every combination and four consecutive iterations, what each
step must contain; the planner and the check are built into one stand-alone program under AddressSanitizer and
UBSan.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chain_planner_sequences_and_invariants(tmp_path):
    exe = tmp_path / "chain_plan_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-I" + csrc, os.path.join(csrc, "ba_chain.cpp"),
                    os.path.join(ROOT, "tests", "native", "chain_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "chain_plan_check OK" in out.stdout
