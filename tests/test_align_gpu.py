"""Alignment of matched landmarks (sg_slam_align_points: k_align_ransac, k_align_select) on the device, and the loop
correction it makes with sg_map_apply_similarity.

The comparators are the planted truth (which matches are wrong, what S_true is) and the numpy references of
tests/align_cases.py (sampler, Horn, residual and MSAC score); never another path of the library.  The bounds come from
tests/test_align_reference_bounds.py (SPREAD_EXACT, MARGIN, NOISY_POSE, no record near the threshold, the gaps of the
hand-built scenes).
"""
import numpy as np
import pytest

import align_cases as ac
import localize_cases as lc
from slamgpu import ba
from slamgpu.scene import quat_to_matrix

pytestmark = pytest.mark.gpu

RESULT_KEYS = ("status", "num_corr", "num_records", "num_inliers", "refined", "best_hypothesis", "best_sample",
               "hypotheses", "models", "msac_cost", "ransac_cost", "inlier_rms", "gap", "scale", "q", "t", "solved",
               "inliers")
MAP_ARRAYS = ("k", "q", "t", "X", "point_flags", "point_uncertainty", "obs_pt", "obs_frame", "obs_point",
              "obs_disabled", "obs_error", "frame_camera", "frame_prev")


def _run(m, groups, slam=None, **kw):
    s = slam or ba.Slam()
    return s.AlignPoints(m, groups, threshold=ac.TAU, **kw)


def _bits(r):
    return tuple(np.asarray(r[k]).tobytes() if not isinstance(r[k], str) else r[k] for k in RESULT_KEYS)


def _arrays(m):
    return {n: getattr(m, n).tobytes() for n in MAP_ARRAYS}


def _check_exact(m, corr, planted, res, kind="sim", seed=ac.SEED):
    """Status, mask, accuracy and sample of one group of an exact scene."""
    ok, X, Y = ac.records(m, corr)
    n = len(X)
    err = ac.result_errors(res, kind)
    R = quat_to_matrix(res["q"])
    e, _, cost = ac.score_np(res["scale"], R, res["t"], X, Y)
    print("N %d, planted %d, %s, h %d, models %d / %d, refined %d, gap %.3f, rotation %.3e deg, translation %.3e, "
          "log scale %.3e, worst true-match residual %.3e" % (n, planted.sum(), res["status"], res["best_hypothesis"],
                                                             res["models"], res["hypotheses"], res["refined"],
                                                             res["gap"], *err, e[~planted].max()))
    assert res["status"] == "OK" and res["solved"] and res["num_records"] == n and res["num_corr"] == len(corr)
    assert np.array_equal(res["inliers"], (~planted).astype(np.int32))
    assert res["num_inliers"] == int((~planted).sum())
    assert ac.within(err, ac.SPREAD_EXACT, ac.MARGIN)
    assert e[~planted].max() <= ac.MARGIN * ac.SPREAD_EXACT["resid"]
    assert abs(res["msac_cost"] - cost) <= 1e-9 * max(cost, 1e-12) + 1e-15
    assert abs(np.linalg.norm(res["q"]) - 1.0) < 1e-14 and res["q"][3] >= 0
    s = res["best_sample"]
    assert len(set(s)) == 3 and not planted[list(s)].any()
    assert s == ac.sample_np(seed, int(corr[0, 0]), res["best_hypothesis"], n)
    assert 0 < res["models"] <= res["hypotheses"] == ac.H
    assert res["gap"] > 100 * ac.MIN_GAP and res["msac_cost"] <= res["ransac_cost"]


@pytest.mark.parametrize("share", [0.0, ac.SHARE])
@pytest.mark.parametrize("kind", ["sim", "rigid"])
def test_exact_scene_mask_accuracy_and_sample(gpu_lib, kind, share):
    m, corr, planted = ac.scene("exact", share, kind)
    base = m.copy()
    res = _run(m, [corr])
    _check_exact(m, corr, planted, res[0], kind)
    assert _arrays(m) == _arrays(base)     # the map is never written


def test_winner_is_the_numpy_argmin(gpu_lib):
    """All 1024 hypotheses of one small noisy group scored in numpy.  (Noisy, because on exact data every all-inlier
    sample's cost is the same double and the order falls to sums of 1e-20 that no two summations round alike.)"""
    m, corr, planted = ac.scene("noisy", ac.SHARE, count=64)
    _, X, Y = ac.records(m, corr)
    n, key = len(X), int(corr[0, 0])
    assert n == 64
    keys = []
    for h in range(ac.H):
        idx = list(ac.sample_np(ac.SEED, key, h, n))
        s, R, t, gap = ac.horn_np(X[idx], Y[idx])
        if not gap > 1e-12:
            continue
        _, inl, cost = ac.score_np(s, R, t, X, Y)
        e2 = ((Y - (s * X @ R.T + t)) ** 2).sum(1)
        keys.append((cost, -int(inl.sum()), float(e2[inl].sum()), h))
    # the documented order: the cost as a double, then more inliers, then the smaller sum over the inliers, then h
    keys.sort()
    best = keys[0]
    res = _run(m, [corr], refine=False)[0]
    print("device h %d, cost %.12g; numpy h %d, cost %.12g, runner-up h %d, cost %.12g" % (
        res["best_hypothesis"], res["ransac_cost"], best[3], best[0], keys[1][3], keys[1][0]))
    assert res["status"] == "OK" and res["refined"] == 0 and res["hypotheses"] == ac.H
    # the same sample drawn twice gives the same key but for h: equal costs are resolved by the smaller h
    tied = [k for k in keys if k[0] <= best[0] * (1 + 1e-9)]
    assert len({tuple(sorted(ac.sample_np(ac.SEED, key, k[3], n))) for k in tied}) == 1, "numpy's minimiser is not unique"
    assert res["best_hypothesis"] == min(k[3] for k in tied)
    assert abs(res["ransac_cost"] - best[0]) <= 1e-9 * best[0] and res["msac_cost"] == res["ransac_cost"]
    assert res["best_sample"] == ac.sample_np(ac.SEED, key, res["best_hypothesis"], n)


@pytest.mark.parametrize("count,share", ac.count_cases())
def test_record_count_boundaries(gpu_lib, count, share):
    m, corr, planted = ac.scene("exact", share, count=count)
    res = _run(m, [corr], min_inliers=4)
    _check_exact(m, corr, planted, res[0])


@pytest.mark.parametrize("share", [0.0, ac.SHARE])
def test_long_group_beyond_the_lds_stage(gpu_lib, share):
    m, corr, planted = ac.long_scene(share)
    res = _run(m, [corr])
    assert res[0]["num_records"] == ac.LONG_COUNT > 1024
    _check_exact(m, corr, planted, res[0])


def test_three_records_do_not_run(gpu_lib):
    m, corr, _ = ac.scene("exact", 0.0, count=3)
    base = m.copy()
    res = _run(m, [corr])[0]
    assert not res["solved"] and res["status"] == "DID_NOT_RUN" and res["num_records"] == 3 == res["num_corr"]
    assert res["best_hypothesis"] == -1 and res["models"] == 0 and (res["inliers"] == -1).all()
    assert res["best_sample"] == (-1, -1, -1) and res["scale"] == 0.0
    assert _arrays(m) == _arrays(base)
    # a fourth correspondence that is no record does not make it run
    m2, corr4, _ = ac.scene("exact", 0.0, count=4)
    m2.point_flags[corr4[3, 1]] = 1 << 0
    res = _run(m2, [corr4])[0]
    assert res["status"] == "DID_NOT_RUN" and res["num_records"] == 3 and res["num_corr"] == 4


def _batch():
    """Four groups of one map: a cut, a group with wrong matches, the tail of the points, and a group of three."""
    m, corr, planted = ac.scene("exact", ac.SHARE)
    return m, [corr[:100], corr[100:300], corr[300:], corr[40:43]]


def test_batch_independence_order_and_reproducibility(gpu_lib):
    m, groups = _batch()
    s = ba.Slam()
    batch = _run(m, groups, slam=s)
    again = _run(m, groups, slam=s)
    assert [_bits(r) for r in batch] == [_bits(r) for r in again]
    assert [r["status"] for r in batch] == ["OK", "OK", "OK", "DID_NOT_RUN"]
    for i, g in enumerate(groups):
        single = _run(m, [g])
        assert _bits(single[0]) == _bits(batch[i]), i
    order = [2, 3, 0, 1]
    shuffled = _run(m, [groups[i] for i in order], slam=s)
    for j, i in enumerate(order):
        assert _bits(shuffled[j]) == _bits(batch[i]), i
    # an unusable correspondence appended to another group changes nothing here
    m.point_flags[groups[2][5, 1]] = 1 << 4
    g1 = np.concatenate([groups[1], groups[2][5:6]])
    other = _run(m, [groups[0], g1], slam=s)
    assert _bits(other[0]) == _bits(batch[0])
    assert other[1]["num_corr"] == 201 and other[1]["num_records"] == 200 and other[1]["inliers"][-1] == -1
    assert np.array_equal(other[1]["inliers"][:-1], batch[1]["inliers"])
    for k in RESULT_KEYS:
        if k not in ("num_corr", "inliers"):
            assert np.array_equal(np.asarray(other[1][k]), np.asarray(batch[1][k])), k


@pytest.mark.parametrize("share", [0.0, ac.SHARE])
@pytest.mark.parametrize("kind", ["sim", "rigid"])
def test_local_optimisation_on_noisy_scenes(gpu_lib, kind, share):
    m, corr, planted = ac.scene("noisy", share, kind)
    fix = kind == "rigid"
    plain = _run(m, [corr], refine=False, fix_scale=fix)[0]
    res = _run(m, [corr], fix_scale=fix)[0]
    err = ac.result_errors(res, kind)
    print("%s share %.1f: refined %d, rotation %.3e deg (bound %.3e), translation %.3e (bound %.3e), log scale %.3e "
          "(bound %.3e), cost %.4f against %.4f, inliers %d against %d" % (
              kind, share, res["refined"], err[0], ac.NOISY_POSE["rot_deg"], err[1], ac.NOISY_POSE["t"], err[2],
              ac.NOISY_POSE["log_scale"], res["msac_cost"], plain["msac_cost"], res["num_inliers"], plain["num_inliers"]))
    assert res["status"] == "OK" and res["solved"]
    assert np.array_equal(res["inliers"], (~planted).astype(np.int32))
    assert res["refined"] >= 1
    assert ac.within(err, ac.NOISY_POSE)
    assert res["msac_cost"] <= res["ransac_cost"] == plain["msac_cost"]
    if fix:
        assert res["scale"] == 1.0 and plain["scale"] == 1.0
    # refine = 0: the reported transform is the winner's, Horn on its three records
    _, X, Y = ac.records(m, corr)
    assert plain["refined"] == 0 and plain["best_hypothesis"] == res["best_hypothesis"]
    idx = list(plain["best_sample"])
    s, R, t, _ = ac.horn_np(X[idx], Y[idx], fix)
    d = ac.score_np(plain["scale"], quat_to_matrix(plain["q"]), plain["t"], X, Y)[0] - ac.score_np(s, R, t, X, Y)[0]
    assert np.abs(d).max() < 1e-6
    # the reported figures are numpy's at the reported transform
    e, inl, cost = ac.score_np(res["scale"], quat_to_matrix(res["q"]), res["t"], X, Y)
    assert abs(res["msac_cost"] - cost) <= 1e-9 * cost
    assert abs(res["inlier_rms"] - np.sqrt((e[inl] ** 2).mean())) <= 1e-9 * res["inlier_rms"]
    gap = ac.horn_np(X[inl], Y[inl], fix)[3]
    assert abs(res["gap"] - gap) <= 1e-9


def test_fix_scale_and_max_scale(gpu_lib):
    m, corr, _ = ac.scene("exact", 0.0, "sim")
    r = _run(m, [corr], fix_scale=True)[0]
    print("fix_scale on the 1.3 scene: %s, %d inliers" % (r["status"], r["num_inliers"]))
    assert r["status"] == "FEW_INLIERS" and not r["solved"] and (r["inliers"] == -1).all() and r["scale"] == 1.0
    r = _run(m, [corr], max_scale=1.1)[0]
    assert r["status"] == "NO_MODEL" and r["models"] == 0 and r["best_hypothesis"] == -1 and r["scale"] == 0.0
    assert r["best_sample"] == (-1, -1, -1) and (r["inliers"] == -1).all()
    r = _run(m, [corr], max_scale=2.0)[0]
    assert r["status"] == "OK" and r["models"] == ac.H and ac.within(ac.result_errors(r), ac.SPREAD_EXACT, ac.MARGIN)
    mr, corr_r, _ = ac.scene("exact", 0.0, "rigid")
    r = _run(mr, [corr_r], fix_scale=True, max_scale=1.0)[0]
    assert r["status"] == "OK" and r["scale"] == 1.0 and ac.within(ac.result_errors(r, "rigid"), ac.SPREAD_EXACT, ac.MARGIN)


def test_hand_built_scenes(gpu_lib):
    m, corr = ac.collinear_scene()
    r = _run(m, [corr])[0]
    print("collinear: %s, models %d" % (r["status"], r["models"]))
    assert r["status"] == "NO_MODEL" and r["models"] == 0
    m, corr = ac.thin_scene()
    r = _run(m, [corr])[0]
    print("thin: %s, models %d, inliers %d, gap %.3e" % (r["status"], r["models"], r["num_inliers"], r["gap"]))
    assert r["status"] == "DEGENERATE" and not r["solved"] and r["num_inliers"] == len(corr)
    assert 1e-12 < r["gap"] < ac.MIN_GAP and (r["inliers"] == -1).all()
    r = _run(m, [corr], min_gap=0.0)[0]          # the gate off: the same group is accepted
    assert r["status"] == "OK" and (r["inliers"] == 1).all()
    m, corr = ac.planar_scene()
    r = _run(m, [corr])[0]
    print("planar: %s, gap %.3f" % (r["status"], r["gap"]))
    assert r["status"] == "OK" and r["num_inliers"] == len(corr) and r["gap"] > 100 * ac.MIN_GAP
    assert ac.within(ac.result_errors(r), ac.SPREAD_EXACT, ac.MARGIN)
    # no similarity joins the two sides, but a proper transform that maps a sample onto its mirror image also fits
    # the few landmarks near the sample's plane: the caller's min_inliers is what refuses such a group.  The tests ask
    # for a quarter of the matches (ac.HAND_MIN_INLIERS_SHARE); numpy's best hypothesis stays far below it
    # (tests/test_align_reference_bounds.py).
    for name in ("mirror", "random"):
        m, corr = getattr(ac, name + "_scene")()
        need = len(corr) // ac.HAND_MIN_INLIERS_SHARE
        r = _run(m, [corr], min_inliers=need)[0]
        print("%s: %s, models %d, inliers %d of %d, %d asked for" % (name, r["status"], r["models"], r["num_inliers"],
                                                                     len(corr), need))
        assert r["status"] == "FEW_INLIERS" and r["num_inliers"] < need and r["models"] > 0 and not r["solved"]
        assert (r["inliers"] == -1).all()


def test_loop_correction_end_to_end(gpu_lib):
    """Frames 5-9 of C1 and the landmarks they see, re-expressed through S_true (points duplicated, the frames'
    observations re-pointed, the frames moved): a drifted submap.  AlignPoints on the matches duplicate -> original
    (30 % of them wrong), then ApplySimilarity, puts it back."""
    base = lc.base_scene("exact")
    s = ba.Slam()
    before = s.ReprojectMap(base.copy())
    frames = np.arange(5, 10, dtype=np.int32)
    in_sub = np.isin(base.obs_frame, frames)
    orig = np.unique(base.obs_point[in_sub]).astype(np.int32)
    m = base.copy()
    dup = ac.append_points(m, ac.apply_true(ac.euclid(base, orig)))
    remap = np.arange(base.num_points)
    remap[orig] = dup
    m.obs_point[in_sub] = remap[base.obs_point[in_sub]].astype(np.int32)
    moved = ac.numpy_apply(m, ac.SCALES["sim"], ac.R_TRUE, ac.T_TRUE, frames, [])
    m.q, m.t = moved.q, moved.t
    drifted = s.ReprojectMap(m.copy())
    # the matches: duplicate -> original, 30 % of them to a wrong original at least 10 TAU from the right one
    rng = np.random.default_rng(31)
    n = len(orig)
    wrong = np.zeros(n, dtype=bool)
    wrong[rng.choice(n, size=int(round(ac.SHARE * n)), replace=False)] = True
    E = ac.euclid(base, orig)
    target = orig.copy()
    for j in np.flatnonzero(wrong):
        far = np.flatnonzero(np.linalg.norm(E - E[j], axis=1) >= 10 * ac.TAU)
        target[j] = orig[rng.choice(far)]
    corr = np.stack([dup, target], 1)
    r = s.AlignPoints(m, [corr], threshold=ac.TAU)[0]
    assert r["status"] == "OK" and np.array_equal(r["inliers"], (~wrong).astype(np.int32))
    s.ApplySimilarity(m, r["scale"], r["q"], r["t"], frames, dup)
    rot = max(ac.rot_err_deg(quat_to_matrix(m.q[4 * f:4 * f + 4]), quat_to_matrix(base.q[4 * f:4 * f + 4]))
              for f in frames)
    dt = np.abs(m.t.reshape(-1, 3)[frames] - base.t.reshape(-1, 3)[frames]).max()
    after = s.ReprojectMap(m)
    print("N %d, %d wrong; frames back within %.3e deg and %.3e; mean reprojection error %.9f px before, %.9f drifted, "
          "%.9f after" % (n, wrong.sum(), rot, dt, before, drifted, after))
    assert rot <= ac.NOISY_POSE["rot_deg"] and dt <= ac.NOISY_POSE["t"]
    assert abs(after - before) <= 1e-6
    assert np.abs(ac.euclid(m, dup) - ac.euclid(base, orig)).max() <= ac.MARGIN * ac.SPREAD_EXACT["resid"]
    keep = np.setdiff1d(np.arange(base.num_frames), frames)
    assert np.array_equal(m.q.reshape(-1, 4)[keep], base.q.reshape(-1, 4)[keep])
    assert np.array_equal(m.X[:4 * base.num_points], base.X)


def test_planner_errors_behind_a_live_handle(gpu_lib):
    m, corr, _ = ac.scene("exact", 0.0, count=16)
    base = m.copy()
    s = ba.Slam()
    s.SolveFrames(lc.base_scene("noisy"), 8, 10, 2.0)      # so that the counters stand somewhere
    assert s.iterations() > 0
    state = (s.iterations(), s.error(), s.last_summary())
    solved_map = _arrays(m)
    bad = corr.copy()
    bad[3, 1] = m.num_points
    same = corr.copy()
    same[2, 1] = same[2, 0]
    for groups, kw in (([bad], {}), ([same], {}), ([corr], {"max_hypotheses": 0}), ([corr], {"min_gap": -1.0}),
                       ([corr], {"max_scale": 0.5}), ([np.array([[-1, 3]])], {})):
        with pytest.raises(Exception):
            s.AlignPoints(m, groups, **kw)
    with pytest.raises(Exception):
        s.AlignPoints(m, [corr], threshold=0.0)
    assert s.AlignPoints(m, []) == []
    assert (s.iterations(), s.error(), s.last_summary()) == state and _arrays(m) == solved_map
    # a good call moves neither the counters nor the map
    r = s.AlignPoints(m, [corr], threshold=ac.TAU)[0]
    assert r["status"] == "OK"
    assert (s.iterations(), s.error(), s.last_summary()) == state and _arrays(m) == solved_map
    assert base.num_points == m.num_points
