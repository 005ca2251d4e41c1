"""Relative pose of frame pairs (sg_slam_relative_poses: k_relpose_ransac, k_relpose_select) on the device.

The comparators are the planted truth (which records are outliers, where frame b really is) and the numpy references
of tests/relpose_cases.py (sampler, normalised 8-point, Sampson score); never another path of the library.  The bounds
come from tests/test_relpose_reference_bounds.py (SPREAD_EXACT, MARGIN, NOISY_POSE, no record near the threshold).
"""
import numpy as np
import pytest

import relpose_cases as rc
from slamgpu import ba
from slamgpu.scene import HEIGHT, WIDTH, quat_to_matrix

pytestmark = pytest.mark.gpu

RESULT_KEYS = ("status", "num_obs", "num_inliers", "num_front", "num_parallax", "refined", "best_hypothesis",
               "best_sample", "hypotheses", "models", "msac_cost", "ransac_cost", "inlier_rms_px", "q", "t", "E")
MAP_ARRAYS = ("k", "q", "t", "X", "point_flags", "point_uncertainty", "obs_pt", "obs_frame", "obs_point",
              "obs_disabled", "obs_error", "frame_camera", "frame_prev")


def _run(m, pairs, slam=None, **kw):
    s = slam or ba.Slam()
    solved = s.RelativePoses(m, pairs, threshold_px=rc.TAU, **kw)
    return solved, s.relative_pose_results(), s.relative_pose_records(), s


def _bits(r):
    return tuple(np.asarray(r[k]).tobytes() if not isinstance(r[k], str) else r[k] for k in RESULT_KEYS)


def _arrays(m, skip=()):
    return {n: getattr(m, n).tobytes() for n in MAP_ARRAYS if n not in skip}


def _errors(m, pair, res):
    R, (Rt, tt, _) = quat_to_matrix(res["q"]), rc.true_rel(m, *pair)
    return rc.rot_err_deg(R, Rt), rc.dir_err_deg(res["t"], tt)


def _check_exact(m, pair, planted, res, recs, i=0, seed=rc.SEED):
    """Status, mask, accuracy and sample of one pair of an exact scene."""
    oa, ob, xa, xb, ka, kb = rc.pair_records(m, *pair)
    n = len(oa)
    off, inl, obs = recs
    rot, dr = _errors(m, pair, res)
    e, _, cost = rc.score_np(res["E"], xa, xb, ka, kb)
    print("pair %s: N %d, planted %d, %s, h %d, models %d / %d, refined %d, rotation %.3e deg, direction %.3e deg, "
          "worst inlier Sampson %.3e px" % (pair, n, planted.sum(), res["status"], res["best_hypothesis"], res["models"],
                                            res["hypotheses"], res["refined"], rot, dr, e[~planted].max()))
    assert res["status"] == "OK" and res["num_obs"] == n == off[i + 1] - off[i]
    assert np.array_equal(inl[off[i]:off[i + 1]], (~planted).astype(np.int32))
    assert np.array_equal(obs[off[i]:off[i + 1]], np.stack([oa, ob], 1))
    assert res["num_inliers"] == res["num_front"] == res["num_parallax"] == int((~planted).sum())
    assert rot <= rc.MARGIN * rc.SPREAD_EXACT["rot_deg"] and dr <= rc.MARGIN * rc.SPREAD_EXACT["dir_deg"]
    assert e[~planted].max() <= rc.MARGIN * rc.SPREAD_EXACT["sampson_px"]
    assert abs(res["msac_cost"] - cost) <= 1e-9 * max(cost, 1e-12) + 1e-15
    assert abs(np.linalg.norm(res["q"]) - 1.0) < 1e-14 and res["q"][3] >= 0
    assert abs(np.linalg.norm(res["t"]) - 1.0) < 1e-14
    assert abs(np.linalg.norm(res["E"]) - np.sqrt(2.0)) < 1e-13
    R = quat_to_matrix(res["q"])
    assert np.abs(res["E"] - rc.skew(-R @ res["t"]) @ R).max() < 1e-9      # E = [t]x R of the reported pose
    s = res["best_sample"]
    assert len(set(s)) == 8 and not planted[list(s)].any()
    assert s == rc.sample_np(seed, rc.pair_key(*pair), res["best_hypothesis"], n)
    assert 0 < res["models"] <= res["hypotheses"] == rc.H


@pytest.mark.parametrize("share", [0.0, rc.SHARE])
@pytest.mark.parametrize("pair", rc.PAIRS)
def test_exact_scene_mask_accuracy_and_sample(gpu_lib, pair, share):
    m, planted = rc.scene("exact", share, pair)
    base = m.copy()
    solved, res, recs, _ = _run(m, [pair])
    assert solved == [True]
    _check_exact(m, pair, planted, res[0], recs)
    assert _arrays(m) == _arrays(base)     # baseline == 0: the map is not written


@pytest.mark.parametrize("count,share", rc.count_cases())
def test_record_count_boundaries(gpu_lib, count, share):
    m, planted = rc.truncated(count, share)
    solved, res, recs, _ = _run(m, [(4, 5)], min_inliers=8)
    assert solved == [True]
    _check_exact(m, (4, 5), planted, res[0], recs)


@pytest.mark.parametrize("share", [0.0, rc.SHARE])
def test_long_pair_beyond_the_lds_stage(gpu_lib, share):
    m, planted = rc.long_scene(share)
    solved, res, recs, _ = _run(m, [rc.LONG_PAIR])
    assert solved == [True] and res[0]["num_obs"] == rc.LONG_COUNT > 1024
    _check_exact(m, rc.LONG_PAIR, planted, res[0], recs)
    assert max(res[0]["best_sample"]) < rc.LONG_COUNT


def test_seven_records_do_not_run(gpu_lib):
    m, _ = rc.truncated(7, 0.0)
    base = m.copy()
    solved, res, recs, _ = _run(m, [(4, 5)], baseline=150.0)
    assert solved == [False] and res[0]["status"] == "DID_NOT_RUN" and res[0]["num_obs"] == 7
    assert res[0]["best_hypothesis"] == -1 and res[0]["models"] == 0 and (recs[1] == -1).all()
    assert _arrays(m) == _arrays(base)


def test_neither_pose_is_read(gpu_lib):
    outs = []
    for garbage in (False, True):
        m, _ = rc.scene("exact", rc.SHARE, (3, 8))
        if garbage:
            rc.garbage_poses(m, [3, 8])
            m.X[:] = np.nan
        outs.append(_bits(_run(m, [(3, 8)])[1][0]))
    assert outs[0] == outs[1]


def test_batch_independence_and_reproducibility(gpu_lib):
    m = rc.batch_scene()
    s = ba.Slam()
    _, batch, recs, _ = _run(m, list(rc.BATCH_PAIRS), slam=s)
    _, again, recs2, _ = _run(m, list(rc.BATCH_PAIRS), slam=s)
    assert [_bits(r) for r in batch] == [_bits(r) for r in again] and np.array_equal(recs[1], recs2[1])
    for i, pair in enumerate(rc.BATCH_PAIRS):
        _, single, rs, _ = _run(m, [pair])
        assert _bits(single[0]) == _bits(batch[i]), pair
        assert np.array_equal(rs[1], recs[1][recs[0][i]:recs[0][i + 1]])


def test_winner_is_the_numpy_argmin(gpu_lib):
    pair = (3, 8)
    m, planted = rc.scene("exact", rc.SHARE, pair)
    oa, _, xa, xb, ka, kb = rc.pair_records(m, *pair)
    costs = np.full(256, np.inf)
    for h in range(256):
        idx = list(rc.sample_np(rc.SEED, rc.pair_key(*pair), h, len(oa)))
        E, _, w = rc.eight_point_np(xa[idx], xb[idx])
        if (w[1] - w[0]) / w[8] > 1e-12:
            costs[h] = rc.score_np(E, xa, xb, ka, kb)[2]
    solved, res, _, _ = _run(m, [pair], max_hypotheses=256, refine=False)
    best = np.flatnonzero(costs <= costs.min() * (1 + 1e-9))
    print("device h %d, numpy minimisers %s, cost %.6g / %.6g" % (res[0]["best_hypothesis"], best, res[0]["msac_cost"],
                                                               costs.min()))
    assert solved == [True] and res[0]["hypotheses"] == 256 and res[0]["refined"] == 0
    assert res[0]["best_hypothesis"] in best


def test_random_pixels_give_few_inliers(gpu_lib):
    m = rc.base_scene("exact")
    _, ob = rc.pair_obs(m, 4, 5)
    rng = np.random.default_rng(5)
    m.obs_pt.reshape(-1, 2)[ob] = rng.uniform((0.0, 0.0), (WIDTH, HEIGHT), size=(len(ob), 2))
    solved, res, recs, _ = _run(m, [(4, 5)])
    print(res[0]["status"], res[0]["num_inliers"])
    assert solved == [False] and res[0]["status"] == "FEW_INLIERS" and res[0]["num_inliers"] < 16
    assert (recs[1] == -1).all()


def test_parallax_count_is_the_numpy_count(gpu_lib):
    """min_parallax in radians, inside pair (4, 5)'s spread: the count is numpy's at the ground truth."""
    m = rc.base_scene("exact")
    want = int((rc.true_parallax(m, 4, 5) >= rc.PARALLAX_GATE).sum())
    solved, res, _, _ = _run(m, [(4, 5)], min_parallax=rc.PARALLAX_GATE)
    print("records with the parallax: %d, numpy %d of %d" % (res[0]["num_parallax"], want, res[0]["num_obs"]))
    assert solved == [True] and res[0]["num_front"] == res[0]["num_inliers"] == res[0]["num_obs"]
    assert res[0]["num_parallax"] == want
    # the same gate with more records required than have the parallax
    solved, res, _, _ = _run(m, [(4, 5)], min_parallax=rc.PARALLAX_GATE, min_inliers=want + 1)
    assert solved == [False] and res[0]["status"] == "LOW_PARALLAX" and res[0]["num_parallax"] == want


def test_almost_pure_rotation_gives_low_parallax(gpu_lib):
    m = rc.near_rotation_scene()
    base = m.copy()
    solved, res, recs, _ = _run(m, [(4, 5)], min_parallax=rc.NEAR_ROTATION_GATE, baseline=150.0)
    rot, dr = _errors(m, (4, 5), res[0])
    print("%s: inliers %d, in front %d, with the parallax %d of %d; rotation %.3e deg, direction %.3e deg" % (
        res[0]["status"], res[0]["num_inliers"], res[0]["num_front"], res[0]["num_parallax"], res[0]["num_obs"], rot, dr))
    assert solved == [False] and res[0]["status"] == "LOW_PARALLAX"
    assert res[0]["num_inliers"] == res[0]["num_front"] == res[0]["num_obs"] and res[0]["num_parallax"] == 0
    assert (recs[1] == -1).all() and _arrays(m) == _arrays(base)      # not solved: nothing written
    solved, res, _, _ = _run(m, [(4, 5)])                             # the gate off: the same pair is accepted
    assert solved == [True] and res[0]["num_parallax"] == res[0]["num_front"]


def test_planar_scene_is_not_ok_with_a_wrong_pose(gpu_lib):
    m = rc.planar_scene()
    solved, res, _, _ = _run(m, [(4, 5)])
    print("planar: %s, models %d of %d, inliers %d" % (res[0]["status"], res[0]["models"], res[0]["hypotheses"],
                                                       res[0]["num_inliers"]))
    if solved == [True]:
        rot, dr = _errors(m, (4, 5), res[0])
        print("rotation %.3e deg, direction %.3e deg" % (rot, dr))
        assert rot <= rc.MARGIN * rc.SPREAD_EXACT["rot_deg"] and dr <= rc.MARGIN * rc.SPREAD_EXACT["dir_deg"]
    else:
        assert res[0]["status"] != "OK"


@pytest.mark.parametrize("share", [0.0, rc.SHARE])
@pytest.mark.parametrize("pair", rc.PAIRS)
def test_local_optimisation_on_noisy_scenes(gpu_lib, pair, share):
    m, planted = rc.scene("noisy", share, pair)
    _, plain, _, _ = _run(m, [pair], refine=False)
    solved, res, recs, _ = _run(m, [pair])
    rot, dr = _errors(m, pair, res[0])
    print("pair %s share %.1f: refined %d, rotation %.3f deg (bound %.3f), direction %.3f deg (bound %.3f), cost %.4f "
          "against %.4f" % (pair, share, res[0]["refined"], rot, 2 * rc.NOISY_POSE[pair][0], dr,
                            2 * rc.NOISY_POSE[pair][1], res[0]["msac_cost"], plain[0]["msac_cost"]))
    assert solved == [True]
    assert np.array_equal(recs[1], (~planted).astype(np.int32))
    assert rot <= 2 * rc.NOISY_POSE[pair][0] and dr <= 2 * rc.NOISY_POSE[pair][1]
    assert res[0]["msac_cost"] <= plain[0]["msac_cost"] == res[0]["ransac_cost"]


def test_writing_frame_b_from_frame_a(gpu_lib):
    m = rc.base_scene("exact")
    rc.garbage_poses(m, [5])
    base = m.copy()
    solved, res, _, _ = _run(m, [(4, 5)], baseline=150.0)
    assert solved == [True]
    centre = np.linalg.norm(m.t[15:18] - m.t_true[15:18])
    rot = rc.rot_err_deg(quat_to_matrix(m.q[20:24]), quat_to_matrix(m.q_true[20:24]))
    print("centre off by %.3e mm, rotation by %.3e deg" % (centre, rot))
    assert abs(rc.true_rel(m, 4, 5)[2] - 150.0) < 1e-9
    assert centre <= np.radians(rc.MARGIN * rc.SPREAD_EXACT["dir_deg"]) * 150.0 + 1e-9
    assert rot <= rc.MARGIN * rc.SPREAD_EXACT["rot_deg"]
    assert abs(np.linalg.norm(m.q[20:24]) - 1.0) < 1e-14 and m.q[23] >= 0
    keep = np.ones(m.num_frames, dtype=bool)
    keep[5] = False
    assert np.array_equal(m.q.reshape(-1, 4)[keep], base.q.reshape(-1, 4)[keep])
    assert np.array_equal(m.t.reshape(-1, 3)[keep], base.t.reshape(-1, 3)[keep])
    assert _arrays(m, skip=("q", "t")) == _arrays(base, skip=("q", "t"))


def test_two_view_bootstrap(gpu_lib):
    """Frame 5's pose and the shared points' locations are garbage; RelativePoses, then TriangulatePoints, bring the
    reprojection error of the pair's records to rounding."""
    m = rc.base_scene("exact")
    oa, ob = rc.pair_obs(m, 4, 5)
    pts = np.unique(m.obs_point[oa])
    rc.garbage_poses(m, [5])
    m.X.reshape(-1, 4)[pts] = (0.5, 0.5, -0.5, 0.5)
    # the bootstrap has two views: the shared points' observations elsewhere are disabled
    other = np.isin(m.obs_point, pts) & ~np.isin(m.obs_frame, (4, 5))
    m.obs_disabled[other] = 1
    s = ba.Slam()
    assert s.RelativePoses(m, [(4, 5)], threshold_px=rc.TAU, baseline=150.0) == [True]
    assert all(s.TriangulatePoints(m, pts))
    s.ReprojectMap(m)
    err = np.linalg.norm(m.obs_error.reshape(-1, 2)[np.concatenate([oa, ob])], axis=1)
    print("mean reprojection error %.3e px over %d observations" % (err.mean(), len(err)))
    assert err.mean() < 1e-6


def test_planner_errors_behind_a_live_handle(gpu_lib):
    m = rc.base_scene("exact")
    s = ba.Slam()
    for pairs in ([(4, 4)], [(4, 10)], [(-1, 5)], [(4, 5), (3, 5)]):
        with pytest.raises(Exception):
            s.RelativePoses(m, pairs)
    assert s.RelativePoses(m, []) == []
