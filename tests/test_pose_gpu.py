"""Pose-only bundle adjustment (sg_slam_solve_frame_poses, k_pose_lm) against the CPU oracle.

Every comparison is with oracle.solve on the per-frame problem built here from the MapArrays: the requested
frame free (rotation and translation), its usable observations in map order, every point constant, and with the
distance term the constant, observation-less previous frame and one FrameDistance block.  The comparator is never
another path of the library."""
import ctypes as C

import numpy as np
import pytest

from slamgpu import ba
from slamgpu.capi import ProblemArrays, default_solver_options
from slamgpu.scene import make_config, make_scene

pytestmark = pytest.mark.gpu

RANGE = 2.0
UNUSABLE = (1 << 0) | (1 << 1) | (1 << 2) | (1 << 4)   # BAD_LOCATION, NO_BASELINE, NO_OBSERVATIONS, BAD_FEATURE
COUNTS = (3, 63, 64, 65, 255, 256, 257, 346)            # wave (64) and workgroup (256) boundaries of k_pose_lm
SUMMARY_INTS = ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps",
                "termination_type", "ok", "num_lm_iterations", "sync_timeouts")
SUMMARY_FLOATS = ("initial_cost", "final_cost", "fixed_cost", "trust_region_radius")

_cache = {}


def _c1():
    if "c1" not in _cache:
        _cache["c1"] = make_config("C1")
    return _cache["c1"].copy()


def _usable_obs(m, f):
    return np.flatnonzero((m.obs_frame == f) & (m.obs_disabled == 0) & ((m.point_flags[m.obs_point] & UNUSABLE) == 0))


def _pose_problem(m, f, with_fd=False):
    """The Ceres problem Slam::SetupProblem would build if only frame f were free, as ProblemArrays."""
    sel = _usable_obs(m, f)
    pts, inv = np.unique(m.obs_point[sel], return_inverse=True)
    prev = int(m.frame_prev[f])
    fd = bool(with_fd) and prev >= 0
    fr = [f, prev] if fd else [f]
    return ProblemArrays(
        k=m.k.copy(), q=m.q.reshape(-1, 4)[fr].copy(), t=m.t.reshape(-1, 3)[fr].copy(),
        frame_camera=m.frame_camera[fr], frame_rot_free=[1, 0][:len(fr)], frame_trans_free=[1, 0][:len(fr)],
        X=m.X.reshape(-1, 4)[pts].copy(), point_free=np.zeros(len(pts), dtype=np.uint8),
        obs_pt=m.obs_pt.reshape(-1, 2)[sel].copy(), obs_frame=np.zeros(len(sel), dtype=np.int32), obs_point=inv,
        dist_frame=[0] if fd else [], dist_prev=[1] if fd else [], range_=RANGE, frame_map_index=fr, point_map_index=pts)


def _oracle(oracle_lib, m, f, options=None, with_fd=False):
    pa = _pose_problem(m, f, with_fd)
    s = oracle_lib.solve(pa, options or default_solver_options())
    return s, pa


def _residuals(oracle_lib, m, f, q, t):
    pa = _pose_problem(m, f)
    pa.q[:4], pa.t[:3] = q, t
    r, _, nf = oracle_lib.evaluate(pa)
    assert nf == 0
    return r


def _gpu(m, frames, options=None, with_fd=False, slam=None):
    s = slam or ba.Slam(options=options)
    solved = s.SolveFramePoses(m, frames, RANGE, with_fd)
    return solved, s.frame_pose_summaries()


def _pose(m, f):
    return m.q[4 * f:4 * f + 4].copy(), m.t[3 * f:3 * f + 3].copy()


def _truncated(count):
    """C1 with frame 8 cut to its first `count` usable observations and started 60 mm off in x."""
    m = _c1()
    sel = _usable_obs(m, 8)
    assert len(sel) == 346
    m.obs_disabled[sel[count:]] = 1
    m.t[3 * 8] += 60.0
    return m


def _oracle_truncated(oracle_lib, count, iters):
    key = ("trunc", count, iters)
    if key not in _cache:
        o = default_solver_options(max_num_iterations=iters) if iters else default_solver_options()
        _cache[key] = _oracle(oracle_lib, _truncated(count), 8, o)
    return _cache[key]


def _assert_same_minimum(oracle_lib, m, f, solved, sg, so, po):
    """The bounds of tests/test_ba_gpu.py's _assert_same_minimum on one frame's pose."""
    q, t = _pose(m, f)
    rg, ro = _residuals(oracle_lib, m, f, q, t), _residuals(oracle_lib, m, f, po.q[:4], po.t[:3])
    print("frame %d: cost %.3e rel, rms %.3e px, t %.3e mm, q %.3e; %s / %s" % (
        f, abs(sg["final_cost"] - so["final_cost"]) / so["final_cost"],
        abs(np.sqrt((rg ** 2).mean()) - np.sqrt((ro ** 2).mean())), np.abs(t - po.t[:3]).max(),
        np.abs(q - po.q[:4]).max(), sg["termination"], so["termination"]))
    assert solved and sg["ok"] == so["ok"] == 1
    assert sg["sync_timeouts"] == 0
    assert sg["termination"] == so["termination"] or {sg["termination"], so["termination"]} <= {
        "FUNCTION_TOLERANCE", "PARAMETER_TOLERANCE", "GRADIENT_TOLERANCE"}
    assert abs(sg["initial_cost"] - so["initial_cost"]) <= 1e-10 * so["initial_cost"]
    assert sg["fixed_cost"] == so["fixed_cost"] == 0.0
    assert abs(sg["final_cost"] - so["final_cost"]) <= 1e-6 * so["final_cost"]
    assert abs(np.sqrt((rg ** 2).mean()) - np.sqrt((ro ** 2).mean())) <= 1e-4
    np.testing.assert_allclose(t, po.t[:3], rtol=0, atol=1e-2)
    np.testing.assert_allclose(q, po.q[:4], rtol=0, atol=1e-6)


@pytest.mark.parametrize("count", COUNTS[1:])
def test_first_5_iterations_match_oracle(gpu_lib, oracle_lib, count):
    """Frame 8 of C1 cut to 63 .. 346 observations (one short of a wave, a wave, one more; the same around the
    256-thread workgroup; every observation), started 60 mm off: the first 5 LM iterations against the oracle,
    step for step, with the bounds of test_c1_first_10_iterations_match_oracle: cost 1e-12 relative, rotation
    1e-9, translation 1e-9 mm.  (The 3-observation case runs to cost 0 and is compared at convergence only.)"""
    o = default_solver_options(max_num_iterations=5)
    so, po = _oracle_truncated(oracle_lib, count, 5)
    m = _truncated(count)
    solved, sums = _gpu(m, [8], o)
    sg = sums[0]
    q, t = _pose(m, 8)
    print("count %d: cost %.3e rel, q %.3e, t %.3e mm" % (
        count, abs(sg["final_cost"] - so["final_cost"]) / so["final_cost"], np.abs(q - po.q[:4]).max(),
        np.abs(t - po.t[:3]).max()))
    assert solved == [True] and sg["ok"] == so["ok"] == 1
    assert sg["termination"] == so["termination"]
    assert sg["num_successful_steps"] == so["num_successful_steps"] == 5
    assert sg["num_unsuccessful_steps"] == so["num_unsuccessful_steps"] == 0
    assert sg["num_iterations"] == so["num_iterations"]
    assert abs(sg["final_cost"] - so["final_cost"]) <= 1e-12 * so["final_cost"]
    np.testing.assert_allclose(q, po.q[:4], rtol=0, atol=1e-9)
    np.testing.assert_allclose(t, po.t[:3], rtol=0, atol=1e-9)


@pytest.mark.parametrize("count", COUNTS)
def test_converged_solve_matches_oracle(gpu_lib, oracle_lib, count):
    """The same truncations solved to convergence with the default options.  With 3 observations the pose is only
    weakly determined (six equations, six unknowns, cost -> 0): ok, the termination and the residuals (1e-6 px)
    are compared, not the pose."""
    so, po = _oracle_truncated(oracle_lib, count, 0)
    m = _truncated(count)
    solved, sums = _gpu(m, [8])
    sg = sums[0]
    if count >= 63:
        _assert_same_minimum(oracle_lib, m, 8, solved[0], sg, so, po)
        return
    q, t = _pose(m, 8)
    rg, ro = _residuals(oracle_lib, m, 8, q, t), _residuals(oracle_lib, m, 8, po.q[:4], po.t[:3])
    print("count 3: residuals %.3e px, %s / %s" % (np.abs(rg - ro).max(), sg["termination"], so["termination"]))
    assert solved == [True] and sg["ok"] == so["ok"] == 1
    assert sg["termination"] == so["termination"]
    np.testing.assert_allclose(rg, ro, rtol=0, atol=1e-6)


def _same_bits(a, b):
    return all(a[k] == b[k] for k in SUMMARY_INTS) and all(
        np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in SUMMARY_FLOATS)


def test_batch_is_independent_and_reproducible(gpu_lib, oracle_lib):
    """All ten C1 frames, each started 60 mm off, in one call against ten oracle solves; the same frames one per
    call, in reversed list order and once more on a copy give the same bits per frame."""
    base = _c1()
    base.t[0::3] += 60.0
    F = base.num_frames
    assert F == 10
    frames = list(range(F))
    mb = base.copy()
    solved, sums = _gpu(mb, frames)
    for f in frames:
        assert len(_usable_obs(base, f)) >= 50   # (frame 0 has the fewest: all well determined)
        so, po = _oracle(oracle_lib, base, f)   # against the map as it was at entry
        _assert_same_minimum(oracle_lib, mb, f, solved[f], sums[f], so, po)
    # one per call (each against the entry map, as the batch solves them)
    for f in frames:
        m1 = base.copy()
        s1, u1 = _gpu(m1, [f])
        assert s1 == [solved[f]] and _same_bits(u1[0], sums[f])
        assert m1.q[4 * f:4 * f + 4].tobytes() == mb.q[4 * f:4 * f + 4].tobytes()
        assert m1.t[3 * f:3 * f + 3].tobytes() == mb.t[3 * f:3 * f + 3].tobytes()
    mr = base.copy()
    sr, ur = _gpu(mr, frames[::-1])
    assert sr == solved[::-1] and all(_same_bits(ur[F - 1 - f], sums[f]) for f in frames)
    assert mr.q.tobytes() == mb.q.tobytes() and mr.t.tobytes() == mb.t.tobytes()
    m2 = base.copy()
    s2, u2 = _gpu(m2, frames)
    assert s2 == solved and all(_same_bits(u2[f], sums[f]) for f in frames)
    assert m2.q.tobytes() == mb.q.tobytes() and m2.t.tobytes() == mb.t.tobytes()


def test_long_frame_beyond_the_lds_stage(gpu_lib, oracle_lib):
    """A frame with 5588 observations: more than the 1024 records k_pose_lm keeps in LDS (kPoseStage), so most
    are re-read from global memory in every sweep."""
    m = make_scene(4, 6000, 11)
    n = len(_usable_obs(m, 2))
    assert n == 5588 and n > 1024
    so, po = _oracle(oracle_lib, m, 2)
    mg = m.copy()
    solved, sums = _gpu(mg, [2])
    _assert_same_minimum(oracle_lib, mg, 2, solved[0], sums[0], so, po)


def test_frame_distance(gpu_lib, oracle_lib):
    """FrameDistance(150) + CauchyLoss(15) to the previous frame's constant translation, against the two-frame
    oracle problem; without a previous frame the flag changes nothing, bit for bit."""
    base = _c1()
    base.t[0::3] += 60.0
    costs = {}
    for f in (3, 9):
        assert base.frame_prev[f] >= 0
        so, po = _oracle(oracle_lib, base, f, with_fd=True)
        m = base.copy()
        solved, sums = _gpu(m, [f], with_fd=True)
        _assert_same_minimum(oracle_lib, m, f, solved[0], sums[0], so, po)
        m0 = base.copy()
        _, sums0 = _gpu(m0, [f], with_fd=False)
        costs[f] = (sums[0]["final_cost"], sums0[0]["final_cost"])
        np.testing.assert_array_equal(m.t[3 * base.frame_prev[f]:][:3], base.t[3 * base.frame_prev[f]:][:3])
    print("final cost with / without the distance term:", costs)
    assert costs[9][0] > costs[9][1] * (1 + 1e-5)   # on frame 9 the term moves the cost
    noprev = base.copy()
    noprev.frame_prev[3] = -1
    ma, mb = noprev.copy(), noprev.copy()
    sa, ua = _gpu(ma, [3], with_fd=True)
    sb, ub = _gpu(mb, [3], with_fd=False)
    assert sa == sb == [True] and _same_bits(ua[0], ub[0])
    assert ma.q.tobytes() == mb.q.tobytes() and ma.t.tobytes() == mb.t.tobytes()


def test_behind_camera_start_fails_and_keeps_the_pose(gpu_lib, oracle_lib):
    base = _c1()
    base.q[12:16] = (0.0, 1.0, 0.0, 0.0)   # frame 3 turned about: everything behind the camera
    so, _ = _oracle(oracle_lib, base, 3)
    assert so["ok"] == 0 and so["termination"] == "NUMERICAL_FAILURE"
    m = base.copy()
    solved, sums = _gpu(m, [3])
    assert solved == [False]
    assert sums[0]["ok"] == 0 and sums[0]["termination"] == "NUMERICAL_FAILURE"
    assert sums[0]["num_iterations"] == so["num_iterations"] == 0
    assert m.q.tobytes() == base.q.tobytes() and m.t.tobytes() == base.t.tobytes()


def test_rejected_steps_match_oracle(gpu_lib, oracle_lib):
    """Frame 3 started 3000 mm back along z: the oracle rejects steps on the way.  The same accepted and rejected
    counts after 5 iterations, the same minimum at convergence."""
    base = _c1()
    base.t[3 * 3 + 2] -= 3000.0
    o = default_solver_options(max_num_iterations=5)
    so5, _ = _oracle(oracle_lib, base, 3, o)
    m5 = base.copy()
    _, sums5 = _gpu(m5, [3], o)
    print("5 iterations: gpu %s, oracle %s" % (sums5[0], so5))
    assert so5["num_unsuccessful_steps"] > 0
    for key in ("num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps", "num_iterations",
                "termination"):
        assert sums5[0][key] == so5[key], key
    so, po = _oracle(oracle_lib, base, 3)
    assert so["num_unsuccessful_steps"] == 5
    m = base.copy()
    solved, sums = _gpu(m, [3])
    _assert_same_minimum(oracle_lib, m, 3, solved[0], sums[0], so, po)
    assert sums[0]["num_unsuccessful_steps"] == so["num_unsuccessful_steps"]


def _others(m):
    return {n: getattr(m, n).tobytes() for n in ("k", "X", "point_flags", "point_uncertainty", "obs_pt", "obs_frame",
                                                 "obs_point", "obs_disabled", "obs_error", "frame_camera",
                                                 "frame_prev")}


def test_nothing_else_moves(gpu_lib):
    base = _c1()
    base.t[0::3] += 60.0
    # frame 5 keeps 2 usable observations: not solved
    base.obs_disabled[_usable_obs(base, 5)[2:]] = 1
    m = base.copy()
    s = ba.Slam()
    solved, sums = _gpu(m, [2, 5, 7], with_fd=True, slam=s)
    assert solved == [True, False, True]
    assert sums[1]["termination"] == "DID_NOT_RUN" and sums[1]["ok"] == 0 and sums[1]["num_iterations"] == 0
    assert _others(m) == _others(base)
    moved = np.zeros(base.num_frames, dtype=bool)
    moved[[2, 7]] = True
    qm, qb = m.q.reshape(-1, 4), base.q.reshape(-1, 4)
    tm, tb = m.t.reshape(-1, 3), base.t.reshape(-1, 3)
    assert qm[~moved].tobytes() == qb[~moved].tobytes() and tm[~moved].tobytes() == tb[~moved].tobytes()
    assert np.abs(tm[moved] - tb[moved]).max() > 1.0   # the requested frames did move
    # a duplicate index: SG_EINVAL and nothing changed
    before = (m.q.tobytes(), m.t.tobytes(), _others(m), s.iterations())
    fr = np.array([2, 7, 2], dtype=np.int32)
    out = np.full(3, 7, dtype=np.int32)
    ms = m.struct()
    rc = s.lib.sg_slam_solve_frame_poses(s.h, C.byref(ms), fr.ctypes.data_as(C.POINTER(C.c_int32)), 3, RANGE, 0,
                                         out.ctypes.data_as(C.POINTER(C.c_int32)), None)
    assert rc == -22
    fr[2] = base.num_frames
    assert s.lib.sg_slam_solve_frame_poses(s.h, C.byref(ms), fr.ctypes.data_as(C.POINTER(C.c_int32)), 3, RANGE, 0,
                                           out.ctypes.data_as(C.POINTER(C.c_int32)), None) == -22
    assert (m.q.tobytes(), m.t.tobytes(), _others(m), s.iterations()) == before


def test_slam_bookkeeping_and_solver_undisturbed(gpu_lib):
    base = _c1()
    base.t[0::3] += 60.0
    base.obs_disabled[_usable_obs(base, 9)[2:]] = 1   # the last listed frame does not run
    s = ba.Slam()
    assert s.iterations() == 0
    m = base.copy()
    solved, sums = _gpu(m, [4, 6, 9], slam=s)
    assert solved == [True, True, False]
    assert s.iterations() == sums[0]["num_iterations"] + sums[1]["num_iterations"] > 2
    assert s.error() == sums[1]["final_cost"]
    assert s.last_summary() == sums[1]
    assert s.SolveFramePose(None, None) is False   # the reference's dead entry stays as it is
    # a window solve on the same handle still matches a fresh handle's, bit for bit
    it0 = s.iterations()
    ma, mb = _c1(), _c1()
    fresh = ba.Slam()
    assert s.SolveFrames(ma, 2, 5, RANGE) == fresh.SolveFrames(mb, 2, 5, RANGE) is True
    assert s.last_summary() == fresh.last_summary()
    assert s.iterations() - it0 == fresh.iterations()
    assert ma.q.tobytes() == mb.q.tobytes() and ma.t.tobytes() == mb.t.tobytes() and ma.X.tobytes() == mb.X.tobytes()
