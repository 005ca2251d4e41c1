"""CPU check of the epipolar matching planner (csrc/epipolar_plan.cpp): tests/native/epipolar_plan_check.cpp plans
generated maps and recomputes by brute force the pair records, the preparation, work and merge lists with the layout of
the partial results, the 128 MiB cap, ResolveEpipolar against a restatement of the acceptance and uniqueness rule, the
CPU executor against an independent double loop, the padding record against the gate, the empty shapes, and every
SG_EINVAL case of the contract.  The planner (with match_plan.cpp, whose ResolveMatches it reuses) and the check are
built into one stand-alone program under AddressSanitizer and UBSan.  The constants that epipolar_cases.py restates
are held equal to the header's.  No GPU, no HIP."""
import os
import re
import subprocess

import epipolar_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_epipolar_planner_matches_brute_force(tmp_path):
    exe = tmp_path / "epipolar_plan_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wno-unknown-pragmas", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "epipolar_plan.cpp"),
                    os.path.join(csrc, "match_plan.cpp"), os.path.join(ROOT, "tests", "native", "epipolar_plan_check.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "epipolar_plan_check OK" in out.stdout
    consts = re.search(r"kEpiChunk (\d+) kEpiTile (\d+) kEpiSlice (\d+) kEpiKeyShift (\d+)", out.stdout)
    assert consts, out.stdout
    chunk, tile, slice_len, shift = map(int, consts.groups())
    assert (chunk, tile, slice_len) == (ec.CHUNK, ec.TILE, ec.SLICE)
    assert slice_len % tile == 0 and shift == 22
