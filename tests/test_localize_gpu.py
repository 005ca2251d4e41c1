"""Localization from scratch (sg_slam_localize_frames: k_pose_ransac, k_pose_select, then k_pose_lm) on the device.

The comparators are the planted truth (which records are outliers, where the frame really is), the numpy references of
tests/localize_cases.py (sampler, Newton P3P, scorer) and oracle.solve on the per-frame problem; never another path of
the library.  The bounds come from tests/test_localize_reference_bounds.py (SPREAD_EXACT_PX, MARGIN, no record near
the threshold) and, for the polish, from tests/test_pose_gpu.py's _assert_same_minimum (same start, same problem)."""
import ctypes as C

import numpy as np
import pytest

import localize_cases as lc
from slamgpu import ba

pytestmark = pytest.mark.gpu

RESULT_KEYS = ("status", "num_obs", "num_inliers", "refined", "best_hypothesis", "best_sample", "hypotheses", "models",
               "msac_cost", "inlier_rms_px", "ransac_cost", "q", "t")


def _run(m, frames, slam=None, **kw):
    s = slam or ba.Slam()
    solved = s.LocalizeFrames(m, frames, threshold_px=lc.TAU, **kw)
    return solved, s.localization_results(), s.localization_inliers(), s


def _pose(m, f):
    return m.q[4 * f:4 * f + 4].copy(), m.t[3 * f:3 * f + 3].copy()


def _bits(r):
    return tuple(np.asarray(r[k]).tobytes() if not isinstance(r[k], str) else r[k] for k in RESULT_KEYS)


def _others(m):
    return {n: getattr(m, n).tobytes() for n in ("k", "X", "point_flags", "point_uncertainty", "obs_pt", "obs_frame",
                                                 "obs_point", "obs_disabled", "obs_error", "frame_camera",
                                                 "frame_prev")}


def _check_exact(m, f, planted, res, inl, seed=0):
    """Status, mask, accuracy and sample of one frame of an exact scene after a refine=0 call."""
    sel, pt, X, k = lc.frame_records(m, f)
    n = len(sel)
    e, _, cost = lc.score_np(*_pose(m, f), k, X, pt)
    worst = e[~planted].max()
    print("frame %d: N %d, planted %d, %s, h %d sample %s, models %d / %d, worst inlier error %.3e px (bound %.3e), "
          "rms %.3e" % (f, n, planted.sum(), res["status"], res["best_hypothesis"], res["best_sample"], res["models"],
                        res["hypotheses"], worst, lc.MARGIN * lc.SPREAD_EXACT_PX, res["inlier_rms_px"]))
    assert res["status"] == "OK" and res["num_obs"] == n and res["refined"] == 0
    assert np.array_equal(inl[sel], (~planted).astype(np.int32))
    assert res["num_inliers"] == int((~planted).sum())
    assert worst <= lc.MARGIN * lc.SPREAD_EXACT_PX
    assert abs(res["msac_cost"] - cost) <= 1e-9 * max(cost, 1e-12) + 1e-18
    assert res["msac_cost"] == res["ransac_cost"]
    assert np.array_equal(_pose(m, f)[0], res["q"]) and np.array_equal(_pose(m, f)[1], res["t"])
    assert abs(np.linalg.norm(res["q"]) - 1.0) < 1e-14 and res["q"][3] >= 0
    s = res["best_sample"]
    assert len(set(s)) == 3 and not planted[list(s)].any()
    assert s == lc.sample_np(seed, f, res["best_hypothesis"], n)
    assert 0 < res["models"] <= res["hypotheses"]


# ---------------------------------------------------------------------------------------------- 1. exact scenes
@pytest.mark.parametrize("share", [0.0, 0.3, 0.6])
def test_exact_scene_mask_accuracy_and_sample(gpu_lib, share):
    m, masks = lc.scene("exact", share)
    base = m.copy()
    solved, res, inl, _ = _run(m, list(lc.FRAMES), refine=False, max_hypotheses=256)
    assert solved == [True, True]
    for i, f in enumerate(lc.FRAMES):
        assert res[i]["hypotheses"] == 256
        _check_exact(m, f, masks[f], res[i], inl)
    listed = np.isin(m.obs_frame, lc.FRAMES)
    assert (inl[~listed] == -1).all() and (inl[listed] >= 0).all()
    assert _others(m) == _others(base)


# ---------------------------------------------------------------------------------------------- 2. record counts
@pytest.mark.parametrize("count,share", [(c, s) for c in lc.COUNTS for s in ((0.0, 0.3) if c >= 63 else (0.0,))])
def test_record_count_boundaries(gpu_lib, count, share):
    """Frame 8 of C1 cut to 4, 5 (the run rule), around a wave (64) and the workgroup (256), and whole."""
    m, planted = lc.truncated(count, share)
    solved, res, inl, _ = _run(m, [8], refine=False, max_hypotheses=256, min_inliers=4)
    assert solved == [True]
    _check_exact(m, 8, planted, res[0], inl)


@pytest.mark.parametrize("share", [0.0, 0.3])
def test_long_frame_beyond_the_lds_stage(gpu_lib, share):
    """5588 records: more than the 1024 k_pose_ransac keeps in LDS (kPoseStage); the rest is read from global
    memory, by the sampler and by every scoring loop."""
    m, planted = lc.long_scene(share)
    solved, res, inl, _ = _run(m, [lc.LONG_FRAME], refine=False, max_hypotheses=256)
    assert solved == [True] and res[0]["num_obs"] == lc.LONG_COUNT > 1024
    _check_exact(m, lc.LONG_FRAME, planted, res[0], inl)
    assert max(res[0]["best_sample"]) < lc.LONG_COUNT


def test_three_records_do_not_run(gpu_lib):
    m, _ = lc.truncated(3, 0.0)
    base = m.copy()
    s = ba.Slam()
    solved, res, inl, _ = _run(m, [8], slam=s, min_inliers=4)
    assert solved == [False] and res[0]["status"] == "DID_NOT_RUN" and res[0]["num_obs"] == 3
    assert res[0]["best_hypothesis"] == -1 and res[0]["models"] == 0 and res[0]["refined"] == 0
    assert (inl == -1).all()
    assert m.q.tobytes() == base.q.tobytes() and m.t.tobytes() == base.t.tobytes() and _others(m) == _others(base)
    assert s.frame_pose_summaries()[0]["termination"] == "DID_NOT_RUN" and s.iterations() == 0


# ---------------------------------------------------------------------------------------------- 3. the entry pose
def test_entry_pose_is_not_read(gpu_lib):
    outs = []
    for entry in ("nan", "identity", "truth", "garbage"):
        m, masks = lc.scene("exact", 0.3, garbage=(entry == "garbage"))
        for f in lc.FRAMES:
            if entry == "nan":
                m.q[4 * f:4 * f + 4] = np.nan
                m.t[3 * f:3 * f + 3] = np.nan
            elif entry == "identity":
                m.q[4 * f:4 * f + 4] = (0, 0, 0, 1)
                m.t[3 * f:3 * f + 3] = 0
        solved, res, inl, s = _run(m, list(lc.FRAMES), refine=True, max_hypotheses=256)
        assert solved == [True, True]
        outs.append(([_bits(r) for r in res], inl.tobytes(), m.q.tobytes(), m.t.tobytes(),
                     [sorted(d.items()) for d in s.frame_pose_summaries()]))
    assert all(o == outs[0] for o in outs[1:])


# ---------------------------------------------------------------------------------------------- 4. independence
def test_batch_is_independent_and_reproducible(gpu_lib):
    """Frame 8 alone, first, in the middle and last in a list of all ten C1 frames, and on a second call of the same
    handle: the same bits."""
    base, _ = lc.scene("noisy", 0.3, frames=(8,))
    kw = dict(refine=True, max_hypotheses=256)
    m0 = base.copy()
    s = ba.Slam()
    solved0, res0, inl0, _ = _run(m0, [8], slam=s, **kw)
    assert solved0 == [True] and res0[0]["refined"] == 1
    sel = lc.usable_obs(base, 8)
    want = (_bits(res0[0]), inl0[sel].tobytes(), _pose(m0, 8)[0].tobytes(), _pose(m0, 8)[1].tobytes())
    rest = [f for f in range(10) if f != 8]
    for frames in ([8] + rest, rest[:5] + [8] + rest[5:], rest + [8]):
        m = base.copy()
        solved, res, inl, _ = _run(m, frames, **kw)
        i = frames.index(8)
        assert solved[i] and (_bits(res[i]), inl[sel].tobytes(), _pose(m, 8)[0].tobytes(),
                              _pose(m, 8)[1].tobytes()) == want
    m2 = base.copy()
    solved2, res2, inl2, _ = _run(m2, [8], slam=s, **kw)
    assert (_bits(res2[0]), inl2[sel].tobytes(), _pose(m2, 8)[0].tobytes(), _pose(m2, 8)[1].tobytes()) == want


def test_winner_is_the_numpy_argmin_over_the_hypotheses(gpu_lib):
    """The fixed-order pick, with one slice (256 hypotheses) and with four (1024): on the noisy scene the MSAC costs
    of different samples differ by far more than rounding, so the winner can be restated.  For every hypothesis whose
    numpy-restated sample holds three planted inliers, the pose by p3p_newton_np (from the true depths) and its numpy
    MSAC cost; the device's best_hypothesis is the argmin over h < H, its cost agrees, and no slice boundary shows.
    Another seed moves best_hypothesis and leaves the mask alone."""
    base, masks = lc.scene("noisy", 0.3, frames=(8,))
    planted = masks[8]
    sel, pt, X, k = lc.frame_records(base, 8)
    n = len(sel)
    q_true, t_true = lc.true_pose(base, 8)
    P = X[:, :3] / X[:, 3:4]
    depth = np.linalg.norm(P - t_true, axis=1)
    f_all = lc.bearings_np(k, pt)
    cost = np.full(1024, np.inf)
    for h in range(1024):
        idx = list(lc.sample_np(0, 8, h, n))
        if planted[idx].any():
            continue
        q, t = lc.p3p_newton_np(f_all[idx], P[idx], depth[idx])
        cost[h] = lc.score_np(q, t, k, X, pt)[2]
    best = {}
    for H in (256, 1024):
        m = base.copy()
        solved, res, inl, _ = _run(m, [8], refine=False, max_hypotheses=H)
        r = res[0]
        want = int(np.argmin(cost[:H]))
        second = np.partition(cost[:H], 1)[1]
        print("H %d: device h %d cost %.6f; numpy argmin %d cost %.6f, runner-up %.6f" % (
            H, r["best_hypothesis"], r["ransac_cost"], want, cost[want], second))
        assert second - cost[want] > 1e-6            # the restated winner is not a matter of rounding
        assert solved == [True] and r["hypotheses"] == H
        assert r["best_hypothesis"] == want
        assert abs(r["ransac_cost"] - cost[want]) <= 1e-6
        assert np.array_equal(inl[sel], (~planted).astype(np.int32))
        best[H] = r
    assert best[1024]["ransac_cost"] <= best[256]["ransac_cost"]
    m = base.copy()
    solved, res, inl, _ = _run(m, [8], refine=False, max_hypotheses=1024, seed=12345)
    assert solved == [True] and res[0]["best_hypothesis"] != best[1024]["best_hypothesis"]
    assert res[0]["best_sample"] == lc.sample_np(12345, 8, res[0]["best_hypothesis"], n)
    assert np.array_equal(inl[sel], (~planted).astype(np.int32))


# ---------------------------------------------------------------------------------------------- 5. statuses
def test_statuses_on_hand_built_maps(gpu_lib):
    base, _ = lc.scene("exact", 0.0)
    pts = np.unique(base.obs_point[lc.usable_obs(base, 8)])
    X = base.X.reshape(-1, 4)
    # frame 8's points on one line; frame 3's points all farther than the |X.w| limit allows
    line = base.copy()
    Xl = line.X.reshape(-1, 4)
    Xl[pts] = np.stack([np.linspace(-2000.0, 2000.0, len(pts)), np.zeros(len(pts)), np.full(len(pts), 3000.0),
                        np.ones(len(pts))], 1)
    Xl[pts] /= np.linalg.norm(Xl[pts], axis=1, keepdims=True)
    pts3 = np.setdiff1d(np.unique(base.obs_point[lc.usable_obs(base, 3)]), pts)
    far = X[pts3].copy()
    far[:, 3] = 0.5 * lc.PNP_MIN_W
    Xl[pts3] = far
    keep3 = np.isin(line.obs_point[lc.usable_obs(line, 3)], pts3)
    line.obs_disabled[lc.usable_obs(line, 3)[~keep3]] = 1   # frame 3 keeps only records of far points
    assert keep3.sum() >= 8
    before = line.copy()
    s = ba.Slam()
    solved, res, inl, _ = _run(line, [8, 3], slam=s, refine=True, max_hypotheses=256)
    print([(r["status"], r["models"], r["num_obs"]) for r in res])
    assert solved == [False, False]
    assert res[0]["status"] == res[1]["status"] == "NO_MODEL" and res[0]["models"] == res[1]["models"] == 0
    assert res[0]["best_hypothesis"] == -1 and res[0]["best_sample"] == (-1, -1, -1)
    assert (inl == -1).all() and s.iterations() == 0
    assert line.q.tobytes() == before.q.tobytes() and line.t.tobytes() == before.t.tobytes()
    assert _others(line) == _others(before)
    # every pixel random: a pose fits its own three records and little else
    rnd = base.copy()
    lc.plant_outliers(rnd, 8, 1.0, 5)
    before = rnd.copy()
    solved, res, inl, _ = _run(rnd, [8, 3], slam=s, refine=True, max_hypotheses=1024, min_inliers=8)
    print([(r["status"], r["num_inliers"], r["models"]) for r in res])
    assert solved == [False, True] and res[0]["status"] == "FEW_INLIERS" and res[1]["status"] == "OK"
    assert 3 <= res[0]["num_inliers"] < 8 and res[0]["refined"] == 0 and res[0]["best_hypothesis"] >= 0
    sums = s.frame_pose_summaries()
    assert sums[0]["termination"] == "DID_NOT_RUN" and sums[1]["ok"] == 1
    assert (inl[rnd.obs_frame != 3] == -1).all() and (inl[lc.usable_obs(rnd, 3)] == 1).all()
    assert s.iterations() == sums[1]["num_iterations"] and s.last_summary() == sums[1]
    moved = np.zeros(rnd.num_frames, dtype=bool)
    moved[3] = True
    assert rnd.q.reshape(-1, 4)[~moved].tobytes() == before.q.reshape(-1, 4)[~moved].tobytes()
    assert rnd.t.reshape(-1, 3)[~moved].tobytes() == before.t.reshape(-1, 3)[~moved].tobytes()
    assert np.abs(_pose(rnd, 3)[1] - lc.true_pose(rnd, 3)[1]).max() < 1e-3
    assert _others(rnd) == _others(before)
    # a failing call (a frame listed twice, a frame out of range) changes nothing
    m, _ = lc.scene("exact", 0.3)
    snap = (m.q.tobytes(), m.t.tobytes(), _others(m), s.iterations())
    ip = C.POINTER(C.c_int32)
    for bad in ([3, 8, 3], [3, 8, m.num_frames], [3, -1, 8]):
        fr = np.array(bad, dtype=np.int32)
        out = np.full(3, 7, dtype=np.int32)
        inl = np.full(m.num_obs, 7, dtype=np.int32)
        opt = ba.SgLocalizeOptions(threshold_px=4.0, max_hypotheses=256, min_inliers=8, seed=0, refine=1, range=2.0)
        ms = m.struct()
        rc = s.lib.sg_slam_localize_frames(s.h, C.byref(ms), fr.ctypes.data_as(ip), 3, C.byref(opt),
                                           out.ctypes.data_as(ip), None, inl.ctypes.data_as(ip), None)
        assert rc == -22 and (out == 7).all() and (inl == 7).all()
        assert (m.q.tobytes(), m.t.tobytes(), _others(m), s.iterations()) == snap


# ---------------------------------------------------------------------------------------------- 6. the polish
def _assert_polish_reaches_the_oracle_minimum(oracle_lib, m, base, f, planted, res, sg, inl):
    """oracle.solve on frame f's problem, started at the device-reported RANSAC pose, against the written pose: the
    bounds of tests/test_pose_gpu.py's _assert_same_minimum (same start, same problem)."""
    so, qo, to = lc.oracle_pose(oracle_lib, base, f, res["q"], res["t"])
    q, t = _pose(m, f)
    rg, ro = lc.oracle_residuals(oracle_lib, base, f, q, t), lc.oracle_residuals(oracle_lib, base, f, qo, to)
    print("frame %d: h %d, inliers %d / %d, ransac cost %.4f -> %.4f; cost %.3e rel, rms %.3e px, t %.3e mm, q %.3e; "
          "%s / %s; off the truth by %.3f mm" % (
              f, res["best_hypothesis"], res["num_inliers"], res["num_obs"], res["ransac_cost"], res["msac_cost"],
              abs(sg["final_cost"] - so["final_cost"]) / so["final_cost"],
              abs(np.sqrt((rg ** 2).mean()) - np.sqrt((ro ** 2).mean())), np.abs(t - to).max(), np.abs(q - qo).max(),
              sg["termination"], so["termination"], np.abs(t - lc.true_pose(base, f)[1]).max()))
    assert res["status"] == "OK" and sg["ok"] == so["ok"] == 1
    assert sg["sync_timeouts"] == 0
    assert sg["termination"] == so["termination"] or {sg["termination"], so["termination"]} <= {
        "FUNCTION_TOLERANCE", "PARAMETER_TOLERANCE", "GRADIENT_TOLERANCE"}
    assert abs(sg["initial_cost"] - so["initial_cost"]) <= 1e-10 * so["initial_cost"]
    assert sg["fixed_cost"] == so["fixed_cost"] == 0.0
    assert abs(sg["final_cost"] - so["final_cost"]) <= 1e-6 * so["final_cost"]
    assert abs(np.sqrt((rg ** 2).mean()) - np.sqrt((ro ** 2).mean())) <= 1e-4
    np.testing.assert_allclose(t, to, rtol=0, atol=1e-2)
    np.testing.assert_allclose(q, qo, rtol=0, atol=1e-6)
    sel = lc.usable_obs(base, f)
    assert int((inl[sel] != (~planted).astype(np.int32)).sum()) == lc.NOISY_INLIERS_OUTSIDE
    assert res["refined"] == 1 and res["msac_cost"] <= res["ransac_cost"]
    assert res["num_inliers"] == int(inl[sel].sum())


@pytest.mark.parametrize("share", [0.3, 0.6])
def test_polish_reaches_the_oracle_minimum(gpu_lib, oracle_lib, share):
    m, masks = lc.scene("noisy", share)
    base = m.copy()
    s = ba.Slam()
    solved, res, inl, _ = _run(m, list(lc.FRAMES), slam=s, refine=True, max_hypotheses=1024)
    sums = s.frame_pose_summaries()
    assert solved == [True, True]
    for i, f in enumerate(lc.FRAMES):
        _assert_polish_reaches_the_oracle_minimum(oracle_lib, m, base, f, masks[f], res[i], sums[i], inl)
    assert s.iterations() == sums[0]["num_iterations"] + sums[1]["num_iterations"]
    assert s.error() == sums[1]["final_cost"] and s.last_summary() == sums[1]
    assert _others(m) == _others(base)


# ---------------------------------------------------------------------------------------------- 7. why it exists
def test_local_solver_cannot_recover_but_localization_does(gpu_lib, oracle_lib):
    """60 % outliers and a garbage entry pose: SolveFramePoses, a local method, does not reach the truth (this
    documents the gap; it is no bound on that path).  LocalizeFrames lands at the oracle's minimum."""
    m, masks = lc.scene("noisy", 0.6, frames=(8,))
    base = m.copy()
    s = ba.Slam()
    ml = m.copy()
    solved = s.SolveFramePoses(ml, [8], 2.0)
    off = np.abs(_pose(ml, 8)[1] - lc.true_pose(base, 8)[1]).max()
    print("SolveFramePoses from the garbage pose: solved %s, %s, translation off the truth by %.1f mm" % (
        solved, s.frame_pose_summaries()[0]["termination"], off))
    assert solved == [False] or off > 100.0
    solved, res, inl, _ = _run(m, [8], slam=s, refine=True, max_hypotheses=1024)
    assert solved == [True]
    sums = s.frame_pose_summaries()
    _assert_polish_reaches_the_oracle_minimum(oracle_lib, m, base, 8, masks[8], res[0], sums[0], inl)
    assert np.abs(_pose(m, 8)[1] - lc.true_pose(base, 8)[1]).max() < 5.0
