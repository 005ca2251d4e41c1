"""CPU check of the relative-pose arithmetic (csrc/relpose_math.h).  tests/native/relpose_math_check.cpp checks the
sampler against a table printed by the numpy restatement (tests/relpose_cases.py) and for distinct in-range indices at
N = 8, 9, 64, 211, 5000; EssentialFromMoments on the exact well-spread sample of each C1 pair against numpy's
normalised 8-point (np.linalg.eigh, np.linalg.svd), up to sign; the (1, 1, 0) projection; the Sampson distance against
numpy; the decomposition recovering the true (R, t) of the four pairs; and "no model" for two identical records, for
eight records of one plane and for NaN.  The cases travel in a text file this test writes from the numpy references.
The header and the check are built into one stand-alone program under AddressSanitizer and UBSan.  No GPU, no HIP."""
import os
import subprocess

import numpy as np

import relpose_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.220446049250313e-16
TABLE = ((0, rc.pair_key(4, 5), 8), (0, rc.pair_key(4, 5), 9), (7, rc.pair_key(3, 8), 64), (0, rc.pair_key(4, 5), 211),
         (3735928559, rc.pair_key(2, 3), 5000))
TABLE_H = (0, 255, 1023)


def _case_lines(m, pair):
    """One pair of the exact scene, as relpose_math_check.cpp's check_case reads it."""
    oa, ob, xa, xb, ka, kb = rc.pair_records(m, *pair)
    idx = rc.spread_sample(m.obs_pt.reshape(-1, 2)[oa])
    E, _, w = rc.eight_point_np(xa[idx], xb[idx])
    gap = (w[1] - w[0]) / w[8]
    R, t_rel, _ = rc.true_rel(m, *pair)
    # tolerances: the null vector of either solver moves by eps / gap (MARGIN covers the constants: the trace against
    # l8, the scales of the de-normalisation); the pose and the Sampson error get MARGIN times the reference's own
    tol = (rc.MARGIN * EPS / gap, rc.MARGIN * np.radians(rc.SPREAD_EXACT["rot_deg"]),
           rc.MARGIN * np.radians(rc.SPREAD_EXACT["dir_deg"]), rc.MARGIN * rc.SPREAD_EXACT["sampson_px"])
    G = E + 0.05 * np.array([[1.0, -2.0, 0.5], [0.3, 1.5, -1.0], [-0.7, 0.2, 0.9]])   # generic: no record on it
    s2 = rc.sampson_np(G, xa, xb, ka, kb)
    assert np.isfinite(s2).all() and (s2 > 1e-6).all()
    rows = [[len(oa)], xa.ravel(), xb.ravel(), 1.0 / ka[3:5], 1.0 / kb[3:5], idx, E.ravel(), tol, R.ravel(), t_rel,
            G.ravel(), s2]
    return [" ".join(repr(float(v)) for v in row) for row in rows]


def test_relpose_math_native_check(tmp_path):
    exe = tmp_path / "relpose_math_check"
    csrc = os.path.join(ROOT, "slam-robot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Wno-unknown-pragmas", "-I" + csrc, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "relpose_math_check.cpp"), "-o", str(exe)], check=True)
    m = rc.base_scene("exact")
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(["%d" % len(rc.PAIRS)] + [ln for p in rc.PAIRS for ln in _case_lines(m, p)]) + "\n")
    out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "relpose_math_check OK" in out.stdout


def sampler_table() -> str:
    """The rows of kTable in relpose_math_check.cpp, as sample_np gives them."""
    rows = []
    for seed, key, n in TABLE:
        idx = ", ".join("{%s}" % ", ".join(str(i) for i in rc.sample_np(seed, key, h, n)) for h in TABLE_H)
        rows.append("{%du, %du, %d, {%s}}," % (seed, key, n, idx))
    return "\n".join(rows)


def test_native_sampler_table_is_the_numpy_restatement():
    src = " ".join(open(os.path.join(ROOT, "tests", "native", "relpose_math_check.cpp")).read().split())
    for row in sampler_table().split("\n"):
        assert src.count(" ".join(row.split())) == 1, row


def test_numpy_sampler_is_distinct_and_in_range():
    for n in (8, 9, 64, 211, 5000):
        for h in range(1024):
            i = rc.sample_np(3, rc.pair_key(4, 5), h, n)
            assert len(set(i)) == 8 and all(0 <= v < n for v in i)
    assert sorted(rc.sample_np(0, rc.pair_key(4, 5), 0, 8)) == list(range(8))
