"""CPU check of the match-by-projection planner (csrc/match_plan.cpp): tests/native/match_plan_check.cpp plans
generated maps and recomputes by brute force the frame records, the gathered points, the skip_observed exclusion mask
(frames listed twice, disabled observations, unlisted points), the work list of keypoint chunks and the launch shapes;
ResolveMatches against a brute-force restatement of the acceptance and uniqueness rule; the empty shapes; and every
SG_EINVAL case of the contract.  The planner and the check are built into one stand-alone program under
AddressSanitizer and UBSan.  The constants that match_cases.py restates are held equal to the header's.  No GPU, no
HIP."""
import os
import re
import subprocess

import match_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_match_planner_matches_brute_force(tmp_path):
    exe = tmp_path / "match_plan_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "match_plan.cpp"),
                    os.path.join(ROOT, "tests", "native", "match_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "match_plan_check OK" in out.stdout
    consts = re.search(r"kMatchChunk (\d+) kMatchTile (\d+) kMatchSlice (\d+) kMatchKeyShift (\d+)", out.stdout)
    assert consts, out.stdout
    chunk, tile, slice_len, shift = map(int, consts.groups())
    assert (chunk, slice_len) == (mc.CHUNK, mc.SLICE)
    assert slice_len % tile == 0 and shift == 22
