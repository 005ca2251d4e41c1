"""CPU check of the pose-graph arithmetic (csrc/posegraph_math.h).  tests/native/posegraph_math_check.cpp checks
PgEdgeEval's residual, cost and rho' and its analytic 7 x 14 Jacobian against central differences through QuatPlus, on
random edges, with q_e near the identity on both sides of the series switch, near the w = 0 flip on both sides, with
and without fix_scale and the Cauchy loss, and the two branches of the rotation-vector factors at the switch.  The
header and the check are built into one stand-alone program under AddressSanitizer and UBSan.  The numpy reference's
residual is held to the same function through the library-free path: both are checked against central differences of
their own, and tests/test_posegraph_capi.py compares whole solves.  No GPU, no HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_posegraph_math_native_check(tmp_path):
    exe = tmp_path / "posegraph_math_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wno-unknown-pragmas", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "posegraph_math_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "posegraph_math_check OK" in out.stdout
