"""CPU check of the alignment planner (csrc/align_plan.cpp): tests/native/align_plan_check.cpp plans generated maps
(unusable flags, NaN and infinite coordinates, points at infinity, W of either sign and any 4-norm, empty groups, a
group of three) and recomputes the records by brute force; the offsets, the sampler key, the N < 4 rule, the launch
shape and every SG_EINVAL case of the contract.  The numpy restatement of the record rule (align_cases.records) is held
to the same filter on C1.  The planner and the check are built into one stand-alone program under AddressSanitizer and
UBSan.  No GPU, no HIP."""
import os
import subprocess

import numpy as np

import align_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_planner_matches_brute_force(tmp_path):
    exe = tmp_path / "align_plan_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-I" + csrc, "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "align_plan.cpp"),
                    os.path.join(ROOT, "tests", "native", "align_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "align_plan_check OK" in out.stdout


def test_numpy_record_rule_on_flags_nan_and_points_at_infinity():
    m, corr, _ = ac.scene("exact", 0.0, count=12)
    X4 = m.X.reshape(-1, 4)
    m.point_flags[corr[0, 0]] = 1 << 0          # BAD_LOCATION on the a side
    m.point_flags[corr[1, 1]] = 1 << 4          # BAD_FEATURE on the b side
    m.point_flags[corr[2, 0]] = 1 << 3          # MISMATCHED: usable
    X4[corr[3, 1], 1] = np.nan
    X4[corr[4, 0], 3] = np.inf
    X4[corr[5, 1], 3] = 0.0
    X4[corr[6, 0], 3] *= 1e-10                  # |W| < 1e-9 |X|
    X4[corr[7, 0]] *= -250.0                    # another sign and norm: the same Euclidean point
    ok, X, Y = ac.records(m, corr)
    assert list(np.flatnonzero(~ok)) == [0, 1, 3, 4, 5, 6]
    assert len(X) == len(Y) == 6 and np.isfinite(X).all() and np.isfinite(Y).all()
    base, _, _ = ac.scene("exact", 0.0, count=12)
    assert np.allclose(X[1], ac.euclid(base, corr[[7], 0])[0], rtol=1e-15, atol=0)      # record 1 is correspondence 7
