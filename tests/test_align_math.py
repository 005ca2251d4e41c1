"""CPU check of the alignment arithmetic (csrc/align_math.h).  tests/native/align_math_check.cpp checks AlignHorn against
numpy's Horn (tests/align_cases.py: rotation from np.linalg.svd, gap from np.linalg.eigvalsh) on the well-spread sample
of three records and on all records of the exact scenes (similarity and rigid, the rigid ones with fix_scale) and on
all true matches of a noisy scene; q within MARGIN * eps / gap, the rest within MARGIN times the reference's own error;
the residual against numpy; a mirrored copy giving a proper rotation with a large residual; "no model" for collinear,
coincident, NaN and zero-spread inputs and for the scale gate; fix_scale giving a scale of exactly 1.  The cases travel
in a text file this test writes from the numpy references.  The header and the check are built into one stand-alone
program under AddressSanitizer and UBSan.  No GPU, no HIP."""
import os
import subprocess

import numpy as np

import align_cases as ac
from slamgpu.scene import axis_angle, quat_from_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.220446049250313e-16


def _case_lines(X, Y, idx, kind, exact):
    fix = kind == "rigid"
    s, R, t, gap = ac.horn_np(X[idx], Y[idx], fix)
    own = ac.errors(s, R, t, kind) if exact else (0.0, 0.0, 0.0)
    # tolerances: the eigenvector of either solver moves by eps / gap; the translation and the scale get MARGIN times
    # the reference's own error (never below the written SPREAD_EXACT: on the noisy scene the truth does not show it);
    # the gap is a ratio of eigenvalues, each good to a few eps of the largest
    tol = (ac.MARGIN * EPS / gap, ac.MARGIN * max(own[1], ac.SPREAD_EXACT["t"]),
           ac.MARGIN * max(own[2], ac.SPREAD_EXACT["log_scale"]), ac.MARGIN * EPS)
    G = (0.8, axis_angle(np.array([0.2, -0.4, 0.3])), np.array([50.0, 60.0, -70.0]))   # generic: no record fits it
    e, _, _ = ac.score_np(*G, X, Y)
    assert (e > 1.0).all()
    rows = [[len(X), int(fix), len(idx)], np.stack([X, Y], 1).ravel(), idx,
            np.concatenate([[s], quat_from_matrix(R), t, [gap]]), tol, np.concatenate([[G[0]], G[1].ravel(), G[2]]),
            e * e]
    return [" ".join(repr(float(v)) for v in row) for row in rows]


def _cases():
    out = []
    for kind in ("sim", "rigid"):
        m, corr, _ = ac.scene("exact", 0.0, kind)
        _, X, Y = ac.records(m, corr)
        out.append(_case_lines(X, Y, np.arange(len(X)), kind, True))
        out.append(_case_lines(X, Y, np.array(ac.spread_sample(X)), kind, True))
    m, corr, planted = ac.scene("noisy", ac.SHARE)
    _, X, Y = ac.records(m, corr)
    out.append(_case_lines(X, Y, np.flatnonzero(~planted), "sim", False))
    return out


def test_align_math_native_check(tmp_path):
    exe = tmp_path / "align_math_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wno-unknown-pragmas", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "align_math_check.cpp"), "-o", str(exe)], check=True)
    cs = _cases()
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(["%d" % len(cs)] + [ln for c in cs for ln in c]) + "\n")
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "align_math_check OK" in out.stdout


def test_numpy_horn_recovers_the_truth_and_its_gap_is_the_singular_value_ratio():
    m, corr, _ = ac.scene("exact", 0.0)
    _, X, Y = ac.records(m, corr)
    for idx in (np.arange(50), np.array(ac.spread_sample(X))):
        s, R, t, gap = ac.horn_np(X[idx], Y[idx])
        assert ac.within(ac.errors(s, R, t), ac.SPREAD_EXACT, ac.MARGIN)
        x, y = X[idx] - X[idx].mean(0), Y[idx] - Y[idx].mean(0)
        sv = np.linalg.svd(x.T @ y, compute_uv=False)
        assert abs(gap - 2 * (sv[1] + sv[2]) / sv.sum()) < 1e-12
    assert abs(np.linalg.det(ac.R_TRUE) - 1.0) < 1e-15
