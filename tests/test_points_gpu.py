"""Structure-only bundle adjustment (sg_slam_solve_points, k_point_lm) against the CPU oracle.

Every comparison is with oracle.solve on the per-point problem built in points_cases.py from the MapArrays; the
comparator is never another path of the library.  The bounds and their origin are in points_cases.py; each test
prints the worst value of every row before it asserts."""
import ctypes as C

import numpy as np
import pytest

import points_cases as pc
from slamgpu import ba
from slamgpu.capi import default_solver_options
from slamgpu.scene import quat_to_matrix

pytestmark = pytest.mark.gpu

RANGE = pc.RANGE
SUMMARY_INTS = ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps",
                "termination_type", "ok", "num_lm_iterations", "sync_timeouts")
SUMMARY_FLOATS = ("initial_cost", "final_cost", "fixed_cost", "trust_region_radius")


def _gpu(m, points, options=None, slam=None):
    s = slam or ba.Slam(options=options)
    solved = s.SolvePoints(m, points, RANGE)
    return solved, s.point_summaries()


def _X(m, points):
    return m.X.reshape(-1, 4)[np.asarray(points, dtype=np.int64)].copy()


def _same_bits(a, b):
    return all(a[k] == b[k] for k in SUMMARY_INTS) and all(
        np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in SUMMARY_FLOATS)


def _check_failed_points(base, m, points, solved, sums, ref_sums):
    """Points whose oracle solve ends with ok = 0: solved = 0, the same termination, X unchanged bit for bit."""
    failed = [i for i in range(len(points)) if not ref_sums[i]["ok"]]
    for i in failed:
        p = points[i]
        assert solved[i] is False and sums[i]["ok"] == 0
        assert sums[i]["termination"] == ref_sums[i]["termination"]
        assert m.X[4 * p:4 * p + 4].tobytes() == base.X[4 * p:4 * p + 4].tobytes()
    assert [bool(s["ok"]) for s in sums] == solved
    return failed


@pytest.mark.parametrize("name", ["A", "B"])
def test_first_5_iterations_match_oracle(gpu_lib, oracle_lib, name):
    """Every point of the scene from start(m, 1) in one call: the first 5 LM iterations against the oracle, step
    for step."""
    base = pc.started(name)
    points = list(range(base.num_points))
    ref_sums, ref_X = pc.cached_oracle(oracle_lib, name, 5)
    m = base.copy()
    solved, sums = _gpu(m, points, default_solver_options(max_num_iterations=5))
    failed = _check_failed_points(base, m, points, solved, sums, ref_sums)
    print("scene %s: %d points start behind a camera" % (name, len(failed)))
    if name == "B":
        assert len(failed) >= 1
    assert all(s["fixed_cost"] == 0.0 and s["sync_timeouts"] == 0 for s in sums)
    pc.compare_it5("scene %s, device" % name, base, points, sums, _X(m, points), ref_sums, ref_X)


@pytest.mark.parametrize("name", ["A", "B"])
def test_converged_solve_matches_oracle(gpu_lib, oracle_lib, name):
    """The same inputs with the default options.  Raw X is not compared (the homogeneous scale is a gauge and
    drifts by several percent): residuals are, and X[:3] / X[3] is printed for information."""
    base = pc.started(name)
    points = list(range(base.num_points))
    ref_sums, ref_X = pc.cached_oracle(oracle_lib, name, 0)
    if name == "B":   # the rejected / invalid step path is exercised
        assert sum(1 for s in ref_sums if s["num_unsuccessful_steps"] or s["num_invalid_steps"]) >= 30
    m = base.copy()
    solved, sums = _gpu(m, points)
    _check_failed_points(base, m, points, solved, sums, ref_sums)
    X = _X(m, points)
    ok = np.array([bool(s["ok"]) for s in ref_sums])
    print("scene %s: Euclidean location, worst difference %.3e mm" % (
        name, np.abs(X[ok, :3] / X[ok, 3:] - ref_X[ok, :3] / ref_X[ok, 3:]).max()))
    pc.compare_converged("scene %s, device" % name, oracle_lib, base, points, sums, X, ref_sums, ref_X)


def test_batch_is_independent_and_reproducible(gpu_lib):
    """Sub-lists of 1, 7, 8, 9 (around a lane group: kPointGroup = 8 points per wave), 31, 32 and 33 points (around a
    workgroup's 32), the reversed full list and the full list on a copy: every point's X and summary are the bits
    of its result in the full call."""
    base = pc.started("B")
    P = base.num_points
    points = list(range(P))
    mf = base.copy()
    solved, sums = _gpu(mf, points)
    assert sum(solved) > 0.9 * P

    def check(sub):
        m = base.copy()
        s, u = _gpu(m, sub)
        for i, p in enumerate(sub):
            assert s[i] == solved[p] and _same_bits(u[i], sums[p]), p
            assert m.X[4 * p:4 * p + 4].tobytes() == mf.X[4 * p:4 * p + 4].tobytes(), p
        rest = np.setdiff1d(points, sub)
        assert _X(m, rest).tobytes() == _X(base, rest).tobytes()

    for k in (1, 7, 8, 9, 31, 32, 33):
        check(points[100:100 + k])
    check(points[::-1])
    check(points)


def test_too_few_observations(gpu_lib):
    base = pc.started("A")
    for p in (40, 41):   # all but one observation disabled
        base.obs_disabled[pc.enabled_obs(base, p)[1:]] = 1
    m = base.copy()
    solved, sums = _gpu(m, [39, 40, 41, 42])
    assert solved == [True, False, False, True]
    for i in (1, 2):
        assert sums[i]["termination"] == "DID_NOT_RUN" and sums[i]["ok"] == 0 and sums[i]["num_iterations"] == 0
    assert _X(m, [40, 41]).tobytes() == _X(base, [40, 41]).tobytes()
    assert all(sums[i]["ok"] == 1 and sums[i]["num_iterations"] > 1 for i in (0, 3))
    assert np.all(np.any(_X(m, [39, 42]) != _X(base, [39, 42]), axis=1))   # the neighbours did move
    # a call in which nothing runs launches nothing and changes nothing
    m2 = base.copy()
    s = ba.Slam()
    assert s.SolvePoints(m2, [41, 40], RANGE) == [False, False]
    assert m2.X.tobytes() == base.X.tobytes() and s.iterations() == 0


def test_behind_camera_start_fails_and_keeps_the_point(gpu_lib, oracle_lib):
    base = pc.started("A")
    base.X[4 * 17:4 * 17 + 3] *= -1.0
    ref_sums, _ = pc.oracle_points(oracle_lib, base, [17])
    assert ref_sums[0]["ok"] == 0 and ref_sums[0]["termination"] == "NUMERICAL_FAILURE"
    assert ref_sums[0]["num_iterations"] == 0
    m = base.copy()
    solved, sums = _gpu(m, [16, 17, 18])
    assert solved == [True, False, True]
    assert sums[1]["ok"] == 0 and sums[1]["termination"] == "NUMERICAL_FAILURE" and sums[1]["num_iterations"] == 0
    assert _X(m, [17]).tobytes() == _X(base, [17]).tobytes()


def _others(m):
    return {n: getattr(m, n).tobytes() for n in ("k", "q", "t", "point_flags", "point_uncertainty", "obs_pt",
                                                 "obs_frame", "obs_point", "obs_disabled", "obs_error", "frame_camera",
                                                 "frame_prev")}


def test_nothing_else_moves(gpu_lib):
    base = pc.started("A")
    base.point_flags[::3] = (1 << 1) | (1 << 2)   # NO_BASELINE | NO_OBSERVATIONS: not consulted, not written
    listed = [5, 300, 6, 483, 0]
    m = base.copy()
    s = ba.Slam()
    solved, _ = _gpu(m, listed, slam=s)
    assert solved == [True] * 5
    assert _others(m) == _others(base)
    rest = np.setdiff1d(np.arange(base.num_points), listed)
    assert _X(m, rest).tobytes() == _X(base, rest).tobytes()
    assert np.all(np.any(_X(m, listed) != _X(base, listed), axis=1))   # the listed points did move
    # a duplicate or out-of-range index: SG_EINVAL, nothing changed, iterations() unchanged
    before = (m.X.tobytes(), _others(m), s.iterations())
    ms = m.struct()
    out = np.full(3, 7, dtype=np.int32)
    for bad in ([5, 6, 5], [5, 6, base.num_points], [5, -1, 6]):
        pts = np.array(bad, dtype=np.int32)
        rc = s.lib.sg_slam_solve_points(s.h, C.byref(ms), pts.ctypes.data_as(C.POINTER(C.c_int32)), 3, RANGE,
                                        out.ctypes.data_as(C.POINTER(C.c_int32)), None)
        assert rc == -22, bad
    assert (m.X.tobytes(), _others(m), s.iterations()) == before


def test_slam_bookkeeping_and_solvers_undisturbed(gpu_lib):
    base = pc.started("A")
    base.obs_disabled[pc.enabled_obs(base, 9)[1:]] = 1   # the last listed point does not run
    s = ba.Slam()
    assert s.iterations() == 0
    m = base.copy()
    solved, sums = _gpu(m, [4, 6, 9], slam=s)
    assert solved == [True, True, False]
    assert s.iterations() == sums[0]["num_iterations"] + sums[1]["num_iterations"] > 2
    assert s.error() == sums[1]["final_cost"]
    assert s.last_summary() == sums[1]
    # a window solve and a pose solve on the same handle still match a fresh handle's, bit for bit
    it0 = s.iterations()
    ma, mb = pc.scene("A"), pc.scene("A")
    fresh = ba.Slam()
    assert s.SolveFrames(ma, 2, 5, RANGE) == fresh.SolveFrames(mb, 2, 5, RANGE) is True
    assert s.last_summary() == fresh.last_summary()
    assert s.iterations() - it0 == fresh.iterations()
    assert ma.q.tobytes() == mb.q.tobytes() and ma.t.tobytes() == mb.t.tobytes() and ma.X.tobytes() == mb.X.tobytes()
    ma.t[0::3] += 60.0
    mb.t[0::3] += 60.0
    assert s.SolveFramePoses(ma, [3, 8], RANGE) == fresh.SolveFramePoses(mb, [3, 8], RANGE) == [True, True]
    assert s.frame_pose_summaries() == fresh.frame_pose_summaries()
    assert ma.q.tobytes() == mb.q.tobytes() and ma.t.tobytes() == mb.t.tobytes()


def test_seeded_depth_use_case(gpu_lib, oracle_lib):
    """What Matcher::Track leaves behind: every point of the newest frame at 2000 mm along its first observation's
    ray (the frame's pose and k, distortion ignored), carrying NO_BASELINE | NO_OBSERVATIONS."""
    base = pc.scene("A")
    newest = base.num_frames - 1
    points = sorted(set(base.obs_point[base.obs_frame == newest].tolist()))
    assert len(points) > 50
    for p in points:
        o = pc.enabled_obs(base, p)[0]
        f = base.obs_frame[o]
        k = base.k[7 * base.frame_camera[f]:][:7]
        u, v = base.obs_pt[2 * o:2 * o + 2]
        ray = np.array([(u - k[5]) / k[3], (v - k[6]) / k[4], 1.0]) * 2000.0
        Xw = quat_to_matrix(base.q[4 * f:4 * f + 4]).T @ ray + base.t[3 * f:3 * f + 3]
        Xh = np.append(Xw, 1.0)
        base.X[4 * p:4 * p + 4] = Xh / np.linalg.norm(Xh)
        base.point_flags[p] = (1 << 1) | (1 << 2)
    ref_sums, ref_X = pc.oracle_points(oracle_lib, base, points)
    assert sum(s["ok"] for s in ref_sums) > 0.9 * len(points)
    m = base.copy()
    solved, sums = _gpu(m, points)
    _check_failed_points(base, m, points, solved, sums, ref_sums)
    assert m.point_flags.tobytes() == base.point_flags.tobytes()
    pc.compare_converged("seeded depth, device", oracle_lib, base, points, sums, _X(m, points), ref_sums, ref_X)
