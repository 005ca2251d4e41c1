"""Linear multi-view triangulation (sg_slam_triangulate_points, k_point_triangulate) against the numpy reference.

Every comparison is with triangulate_cases.triangulate_np (np.linalg.eigh for the eigen-solve) or, for the polish,
with oracle.solve started from that reference's location; the comparator is never another path of the library.  The
bounds and their origin are in triangulate_cases.py; each comparison prints the worst value of every row before it
asserts."""
import ctypes as C

import numpy as np
import pytest

import points_cases as pc
import triangulate_cases as tc
from slamgpu import ba
from slamgpu.capi import SgTriangulateOptions, default_solver_options
from slamgpu.scene import K_ROBOT, MapArrays

pytestmark = pytest.mark.gpu

RESULT_FLOATS = ("parallax", "max_error_px", "rel_gap")


def _tri(m, points, slam=None, **kw):
    s = slam or ba.Slam()
    solved = s.TriangulatePoints(m, points, **kw)
    return solved, s.triangulation_results()


def _X(m, points):
    return m.X.reshape(-1, 4)[np.asarray(points, dtype=np.int64)].copy()


def _same_bits(a, b):
    return a["status"] == b["status"] and a["num_obs"] == b["num_obs"] and a["X"].tobytes() == b["X"].tobytes() and all(
        np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in RESULT_FLOATS)


def _others(m):
    return {n: getattr(m, n).tobytes() for n in ("k", "q", "t", "point_flags", "point_uncertainty", "obs_pt",
                                                 "obs_frame", "obs_point", "obs_disabled", "obs_error", "frame_camera",
                                                 "frame_prev")}


def _check_write_back(base, m, points, solved, res):
    """solved and the written X are exactly the OK points' (refine = 0); every other X is kept bit for bit."""
    assert solved == [r["status"] == "OK" for r in res]
    for i, p in enumerate(points):
        want = res[i]["X"] if solved[i] else base.X[4 * p:4 * p + 4]
        assert m.X[4 * p:4 * p + 4].tobytes() == want.tobytes(), p
    rest = np.setdiff1d(np.arange(base.num_points), points)
    assert _X(m, rest).tobytes() == _X(base, rest).tobytes()
    assert _others(m) == _others(base)


@pytest.mark.parametrize("name", ["A", "B"])
def test_exact_scenes(gpu_lib, name):
    base = tc.scene(name, exact=True)
    points = list(range(base.num_points))
    m = base.copy()
    solved, res = _tri(m, points)
    assert all(r["status"] == "OK" for r in res) and all(solved)
    err = max(r["max_error_px"] for r in res)
    print("scene %s exact, device: worst max_error_px %.2e" % (name, err))
    assert err <= tc.EXACT_ERROR_PX
    truth = [dict(r, X=base.X_true[4 * p:4 * p + 4]) for p, r in enumerate(tc.reference(name, exact=True))]
    w = tc.spreads(res, truth)
    print("scene %s exact, device against X_true: |dX| rel_gap %.2e; |dX| %.2e" % (name, w["x_gap"], w["x"]))
    assert w["x_gap"] <= tc.MARGIN * tc.SPREAD_X_GAP and w["x"] <= tc.MARGIN * tc.SPREAD_X
    tc.compare("scene %s exact, device" % name, res, tc.reference(name, exact=True))
    _check_write_back(base, m, points, solved, res)


@pytest.mark.parametrize("name", ["A", "B"])
def test_noisy_scenes_with_gates(gpu_lib, name):
    base = tc.scene(name)
    points = list(range(base.num_points))
    ref = tc.reference(name, gates=True)
    m = base.copy()
    solved, res = _tri(m, points, min_parallax=tc.GATE_RAD, max_error_px=tc.GATE_PX)
    near = [p for p in points if abs(ref[p]["max_error_px"] - tc.GATE_PX) <= tc.NEAR_GATE
            or abs(ref[p]["parallax"] - tc.GATE_RAD) <= tc.NEAR_GATE]
    assert len(near) <= tc.NEAR_GATE_POINTS
    differs = [p for p in points if res[p]["status"] != ref[p]["status"] and p not in near]
    st = [r["status"] for r in res]
    print("scene %s noisy, device: %s; status differs on %s" % (name, {k: st.count(k) for k in sorted(set(st))}, differs))
    assert not differs
    assert st.count("HIGH_ERROR") > 0 and st.count("LOW_PARALLAX") > 0
    assert [r["num_obs"] for r in res] == [r["num_obs"] for r in ref]
    tc.compare("scene %s noisy, device" % name, res, ref)
    _check_write_back(base, m, points, solved, res)


def test_entry_location_is_not_read(gpu_lib):
    base = tc.scene("B")
    points = list(range(0, base.num_points, 2))
    ma, mb = base.copy(), base.copy()
    mb.X.reshape(-1, 4)[points] = 0.0
    sa, ra = _tri(ma, points)
    sb, rb = _tri(mb, points)
    assert sa == sb and sum(sa) > 0.9 * len(points)
    assert all(_same_bits(a, b) for a, b in zip(ra, rb))
    assert _X(ma, points)[sa].tobytes() == _X(mb, points)[sb].tobytes()


def _hand_built():
    """Four frames, identity rotations, centres (0,0,0), (0,0,1000), (150,0,0), (0,0,0); pinhole pixels without a
    cheirality test.  Returns the map and the expected status per point."""
    centres = np.array([[0, 0, 0], [0, 0, 1000], [150, 0, 0], [0, 0, 0]], dtype=np.float64)
    cases = [((30, 20, 500), (0, 1), "BEHIND"),            # between the two cameras
             ((100, 50, 2000), (0, 3), "NO_BASELINE"),
             ((100, 50, 2000), (0, 2), "OK"),
             ((100, 50, -2000), (0, 2), "BEHIND"),         # what the W >= 0 rule is for
             ((100, 50, 2000), (0, 2), "DID_NOT_RUN"),     # all but one observation disabled
             ((0, 0, 3000), (0, 1, 0, 1), "DEGENERATE")]   # on the baseline: the same two rays twice, no parallax
    rows = []
    for p, (P, frames, _) in enumerate(cases):
        for f in frames:
            d = np.array(P, dtype=np.float64) - centres[f]
            rows.append((f, p, K_ROBOT[3] * d[0] / d[2] + K_ROBOT[5], K_ROBOT[4] * d[1] / d[2] + K_ROBOT[6]))
    rows.sort(key=lambda r: (r[0], r[1]))
    M, P = len(rows), len(cases)
    X = np.tile(np.array([0.1, 0.2, 0.3, 1.0]) / np.linalg.norm([0.1, 0.2, 0.3, 1.0]), P)
    m = MapArrays(
        k=np.concatenate([K_ROBOT, K_ROBOT]), q=np.tile([0.0, 0.0, 0.0, 1.0], 4), t=centres.reshape(-1).copy(),
        frame_camera=np.array([1, 0, 1, 0], dtype=np.int32), frame_prev=np.arange(-1, 3, dtype=np.int32), X=X,
        point_flags=np.array([0, 2, 4, 6, 0, 1], dtype=np.int32), point_uncertainty=np.ones(P),
        obs_pt=np.array([[r[2], r[3]] for r in rows]).reshape(-1), obs_frame=np.array([r[0] for r in rows], dtype=np.int32),
        obs_point=np.array([r[1] for r in rows], dtype=np.int32), obs_disabled=np.zeros(M, dtype=np.int32),
        obs_error=np.zeros(2 * M))
    m.obs_disabled[pc.enabled_obs(m, 4)[1:]] = 1
    return m, [c[2] for c in cases], [c[0] for c in cases]


def test_statuses_on_a_hand_built_map(gpu_lib):
    base, expected, where = _hand_built()
    points = list(range(base.num_points))
    m = base.copy()
    s = ba.Slam()
    solved, res = _tri(m, points, slam=s)
    assert [r["status"] for r in res] == expected
    assert [r["status"] for r in res] == [tc.triangulate_np(base, p)["status"] for p in points]
    assert solved == [False, False, True, False, False, False]
    _check_write_back(base, m, points, solved, res)
    X = res[2]["X"]
    assert X[3] > 0 and abs(np.linalg.norm(X) - 1.0) <= 4e-16 and np.abs(X[:3] / X[3] - where[2]).max() <= 1e-6
    for i in (0, 3):   # computed, reported, not written
        Xi = res[i]["X"]
        assert Xi[3] > 0 and np.abs(Xi[:3] / Xi[3] - where[i]).max() <= 1e-6
    for i in (1, 4, 5):
        assert not res[i]["X"].any()
    assert [r["num_obs"] for r in res] == [2, 2, 2, 2, 1, 4]
    assert s.iterations() == 0 and all(u["termination"] == "DID_NOT_RUN" for u in s.point_summaries())
    # the gates, in the order of the rules
    for kw, want in ((dict(min_parallax=0.5), "LOW_PARALLAX"), (dict(max_error_px=1e-12, min_parallax=0.5), "LOW_PARALLAX"),
                     (dict(min_parallax=0.01, max_error_px=0.5), "OK")):
        m2 = base.copy()
        solved, res = _tri(m2, [2, 3], slam=s, **kw)
        assert [r["status"] for r in res] == [want, "BEHIND"]
        _check_write_back(base, m2, [2, 3], solved, res)
    # a call in which nothing runs launches nothing and changes nothing
    m3 = base.copy()
    assert s.TriangulatePoints(m3, [4]) == [False] and m3.X.tobytes() == base.X.tobytes()
    # a duplicate or out-of-range index: SG_EINVAL, nothing changed
    ms = m3.struct()
    out = np.full(3, 7, dtype=np.int32)
    opt = SgTriangulateOptions(range=2.0)
    for bad in ([2, 3, 2], [2, 3, base.num_points], [2, -1, 3]):
        pts = np.array(bad, dtype=np.int32)
        rc = s.lib.sg_slam_triangulate_points(s.h, C.byref(ms), pts.ctypes.data_as(C.POINTER(C.c_int32)), 3,
                                              C.byref(opt), out.ctypes.data_as(C.POINTER(C.c_int32)), None, None)
        assert rc == -22, bad
    assert m3.X.tobytes() == base.X.tobytes() and _others(m3) == _others(base) and out.tolist() == [7, 7, 7]


def test_distortion(gpu_lib):
    base = tc.distorted_scene()
    points = list(range(base.num_points))
    m = base.copy()
    solved, res = _tri(m, points)
    assert all(r["status"] == "OK" for r in res)
    err = max(r["max_error_px"] for r in res)
    print("scene A exact, k = (-0.1, 0.02, 0), device: worst max_error_px %.2e" % err)
    assert err <= tc.EXACT_ERROR_PX
    tc.compare("scene A distorted, device", res, [tc.triangulate_np(base, p) for p in points])


def test_batch_is_independent_and_reproducible(gpu_lib):
    """Sub-lists of 1, 7, 8, 9 (around a lane group: 8 points per wave), 31, 32 and 33 points (around a workgroup's
    32), the reversed full list and the full list again: every point's result and written X are the bits of its
    result in the full call."""
    base = tc.scene("B")
    base.obs_disabled[pc.enabled_obs(base, 104)[1:]] = 1   # an idle group among the running ones
    points = list(range(base.num_points))
    kw = dict(min_parallax=tc.GATE_RAD, max_error_px=tc.GATE_PX)
    mf = base.copy()
    solved, res = _tri(mf, points, **kw)
    assert res[104]["status"] == "DID_NOT_RUN" and len(set(r["status"] for r in res)) >= 4

    def check(sub):
        m = base.copy()
        s, r = _tri(m, sub, **kw)
        for i, p in enumerate(sub):
            assert s[i] == solved[p] and _same_bits(r[i], res[p]), p
            assert m.X[4 * p:4 * p + 4].tobytes() == mf.X[4 * p:4 * p + 4].tobytes(), p
        rest = np.setdiff1d(points, sub)
        assert _X(m, rest).tobytes() == _X(base, rest).tobytes()

    for k in (1, 7, 8, 9, 31, 32, 33):
        check(points[100:100 + k])
    check(points[::-1])
    check(points)


def test_polish_from_a_start_solve_points_refuses(gpu_lib, oracle_lib):
    base = pc.started("B", 1)
    points = list(range(base.num_points))
    o5 = default_solver_options(max_num_iterations=5)
    # existing behaviour: the points that start behind a camera stay unsolved
    m0 = base.copy()
    s0 = ba.Slam(options=o5)
    refused = [p for p, ok in zip(points, s0.SolvePoints(m0, points, pc.RANGE)) if not ok]
    print("SolvePoints refuses %s" % refused)
    assert len(refused) == 3
    # the reference: its triangulation, then oracle.solve from there
    ref = [tc.triangulate_np(base, p) for p in points]
    assert all(r["status"] == "OK" for r in ref)
    mr = base.copy()
    mr.X[:] = np.concatenate([r["X"] for r in ref])
    ref_sums, ref_X = pc.oracle_points(oracle_lib, mr, points, o5)
    # the device, without the polish: nothing of the handle moves
    s = ba.Slam(options=o5)
    m1 = base.copy()
    assert all(s.TriangulatePoints(m1, points))
    assert s.iterations() == 0 and all(u["termination"] == "DID_NOT_RUN" for u in s.point_summaries())
    tri = s.triangulation_results()
    tc.compare("started B, device", tri, ref)
    # with the polish
    m = base.copy()
    solved = s.TriangulatePoints(m, points, refine=True, range_=pc.RANGE)
    sums = s.point_summaries()
    assert all(solved) and all(solved[p] for p in refused)
    assert all(_same_bits(a, b) for a, b in zip(s.triangulation_results(), tri))   # X before the polish
    assert s.iterations() == sum(u["num_iterations"] for u in sums) > 2 * len(points)
    assert s.error() == sums[-1]["final_cost"] and s.last_summary() == sums[-1]
    X = _X(m, points)
    lm_failed = [p for p in points if not sums[p]["ok"]]
    print("LM ends with ok = 0 on %s" % lm_failed)
    for p in lm_failed:   # keeps the triangulated location, and stays solved
        assert X[p].tobytes() == tri[p]["X"].tobytes()
    moved = [p for p in points if sums[p]["ok"] and X[p].tobytes() != tri[p]["X"].tobytes()]
    assert len(moved) > 0.9 * len(points)
    assert _others(m) == _others(base)
    pc.compare_it5("started B, polish on the device", base, points, sums, X, ref_sums, ref_X)


def test_solve_points_undisturbed(gpu_lib):
    base = pc.started("A", 1)
    points = list(range(base.num_points))
    fresh, s = ba.Slam(), ba.Slam()
    mf = base.copy()
    want = fresh.SolvePoints(mf, points, pc.RANGE)
    want_sums = fresh.point_summaries()
    ma = base.copy()
    assert s.SolvePoints(ma, points, pc.RANGE) == want and s.point_summaries() == want_sums
    assert ma.X.tobytes() == mf.X.tobytes()
    it = s.iterations()
    assert it == fresh.iterations()
    for kw in (dict(), dict(refine=True)):
        s.TriangulatePoints(base.copy(), points[::3], **kw)
    it2 = s.iterations()
    mb = base.copy()
    assert s.SolvePoints(mb, points, pc.RANGE) == want and s.point_summaries() == want_sums
    assert mb.X.tobytes() == mf.X.tobytes()
    assert s.iterations() - it2 == it and s.last_summary() == fresh.last_summary()
