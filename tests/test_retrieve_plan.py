"""CPU check of the host-only side of the keyframe descriptor database (csrc/retrieve_plan.cpp):
tests/native/retrieve_plan_check.cpp recomputes by brute force the bookkeeping and its caps, the slice work lists (no
slice crosses a set; the slices cover each non-skipped, non-empty set exactly once), the slice length rule and the
launch shapes, the ranking, the CPU executor of rules 1-6 against a second restatement, every SG_EINVAL case and the
empty shapes.  The planner and the check are built into one stand-alone program under AddressSanitizer and UBSan.  The
constants that retrieve_cases.py restates are held equal to the header's.  No GPU, no HIP."""
import os
import re
import subprocess

import retrieve_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_retrieve_planner_matches_brute_force(tmp_path):
    exe = tmp_path / "retrieve_plan_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "retrieve_plan.cpp"),
                    os.path.join(ROOT, "tests", "native", "retrieve_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "retrieve_plan_check OK" in out.stdout
    consts = re.search(r"kRetrieveQ (\d+) kRetrieveTile (\d+) kRetrieveSlice (\d+) kRetrieveClaimShift (\d+)", out.stdout)
    assert consts, out.stdout
    q, tile, slice_len, shift = map(int, consts.groups())
    assert (q, tile, slice_len) == (rc.Q, rc.T, rc.L)
    assert slice_len % tile == 0 and shift == 22
