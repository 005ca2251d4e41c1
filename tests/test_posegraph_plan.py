"""CPU check of the pose-graph planner and its CPU executor (csrc/posegraph_plan.cpp): tests/native/
posegraph_plan_check.cpp plans seeded random calls and recomputes, by brute force, the minimum-degree order, the fill
(a dense boolean elimination in the planned order), the assembly and update lists (every contribution exactly once, no
target twice in a column), the status rules (two components, one without a fixed node), every SG_EINVAL of the contract
and the size caps; and it solves chords24's first linearization with the executor and with a dense Cholesky in long
double, the step held to MARGIN * SPREAD.  The planner and the check are built into one stand-alone program twice:
plain, and under AddressSanitizer and UBSan.  No GPU, no HIP."""
import os
import subprocess

import numpy as np
import pytest

import posegraph_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case_file(path):
    sc = pc.scene("chords24")
    rows = ["%d %d" % (len(sc["q"]), len(sc["edges"]))]
    for q, t, f in zip(sc["q"], sc["t"], sc["fixed"]):
        rows.append(" ".join(repr(float(v)) for v in (*q, *t)) + " %d" % f)
    for (a, b), m, w in zip(sc["edges"], sc["meas"], sc["weights"]):
        rows.append("%d %d " % (a, b) + " ".join(repr(float(v)) for v in (*m, *w)))
    sp = pc.SPREAD["chords24"]
    rows.append(" ".join(repr(float(v)) for v in (pc.MARGIN * np.radians(sp["rot_deg"]), pc.MARGIN * sp["t"],
                                                  pc.MARGIN * sp["log_scale"], pc.OPTIONS["initial_trust_region_radius"])))
    path.write_text("\n".join(rows) + "\n")


@pytest.mark.parametrize("sanitize", [False, True])
def test_posegraph_planner_and_executor(tmp_path, sanitize):
    exe = tmp_path / "posegraph_plan_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Wno-unknown-pragmas", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "posegraph_plan.cpp"),
                    os.path.join(ROOT, "tests", "native", "posegraph_plan_check.cpp"), "-o", str(exe)], check=True)
    cases = tmp_path / "chords24.txt"
    _case_file(cases)
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "posegraph_plan_check OK" in out.stdout and "executor against dense" in out.stdout
