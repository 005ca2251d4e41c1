"""The bounds of the relative-pose tests, from the numpy references of tests/relpose_cases.py alone (no GPU, no
library):

  * COUNTS_C1 and LONG_COUNT: the record counts of the pairs.
  * SPREAD_EXACT: on the exact scenes, the rotation error, the direction error and the worst Sampson error of the
    reference 8-point from one fixed well-spread sample of eight records per pair (spread_sample: the records nearest
    to eight image anchors), over PAIRS.  The code under test is held to MARGIN = 100 times these values.
  * At the reference's all-inlier 8-point from the non-planted records, on every case a mask is checked on: no record
    within NEAR = 1e-6 px of TAU (cap 0); every planted record an outlier; every other record an inlier on the exact
    scenes, and on the noisy ones the count that is not is NOISY_INLIERS_OUTSIDE.
  * For each case with planted outliers, the all-inlier samples among the H hypotheses of seed SEED, counted with the
    numpy sampler, are at least 8 and at least MIN_ALL_INLIER_SAMPLES.
  * NOISY_POSE: the rotation and direction error of that all-inlier estimate on the noisy scenes, per pair.
A written constant must be an upper bound, and within a factor of 4 of the recomputed value.

Planting departs from "uniform in the image" in one way: a record whose pixel in a lies within 60 px of the epipole in
a is never planted, because every epipolar line in a passes through the epipole and the 20 px rule cannot be met
there.  So the almost-forward pair (2, 8), whose epipole is inside the image, never has an outlier near it."""
import numpy as np

import relpose_cases as rc


def _pose_errors(m, pair, E, xa, xb, inl):
    R, t, front, _ = rc.decompose_np(E, xa, xb, inl)
    Rr, tr = rc.rel_from_cv(R, t)
    Rt, tt, _ = rc.true_rel(m, *pair)
    return rc.rot_err_deg(Rr, Rt), rc.dir_err_deg(tr, tt), int(front.sum())


def test_record_counts():
    m = rc.base_scene("exact")
    for pair, n in rc.COUNTS_C1.items():
        assert len(rc.pair_obs(m, *pair)[0]) == n, pair
    assert len(rc.long_scene(0.0)[1]) == rc.LONG_COUNT > 1024


def test_spread_exact_is_the_reference_error():
    worst = {"rot_deg": 0.0, "dir_deg": 0.0, "sampson_px": 0.0}
    m = rc.base_scene("exact")
    for pair in rc.PAIRS:
        oa, _, xa, xb, ka, kb = rc.pair_records(m, *pair)
        idx = rc.spread_sample(m.obs_pt.reshape(-1, 2)[oa])
        E, _, w = rc.eight_point_np(xa[idx], xb[idx])
        e, inl, _ = rc.score_np(E, xa, xb, ka, kb)
        rot, dr, front = _pose_errors(m, pair, E, xa, xb, inl)
        print("pair %s: sample %s, gap %.3e, rotation %.3e deg, direction %.3e deg, worst Sampson %.3e px" % (
            pair, idx, (w[1] - w[0]) / w[8], rot, dr, e.max()))
        assert inl.all() and front == len(oa)
        for key, v in (("rot_deg", rot), ("dir_deg", dr), ("sampson_px", float(e.max()))):
            worst[key] = max(worst[key], v)
    print("recomputed %s, written %s" % (worst, rc.SPREAD_EXACT))
    for key, v in worst.items():
        assert v <= rc.SPREAD_EXACT[key] <= 4.0 * v, key
    assert rc.MARGIN == 100.0


def test_masks_thresholds_sample_counts_and_noisy_pose():
    near = outside = 0
    fewest = rc.H
    noisy = {p: [0.0, 0.0] for p in rc.PAIRS}
    for name, m, pair, planted, exact in rc.all_cases():
        oa, _, xa, xb, ka, kb = rc.pair_records(m, *pair)
        n = len(oa)
        assert len(planted) == n, name
        E, _, w = rc.eight_point_np(xa[~planted], xb[~planted])
        e, inl, _ = rc.score_np(E, xa, xb, ka, kb)
        n_near = int((np.abs(e - rc.TAU) <= rc.NEAR).sum())
        n_out = int((~inl & ~planted).sum())
        line = "%s: N %d, planted %d, near %d, unplanted outside %d, smallest planted error %.2f px, largest other " \
               "%.3e px" % (name, n, planted.sum(), n_near, n_out, e[planted].min() if planted.any() else np.inf,
                            e[~planted].max())
        near += n_near
        assert not inl[planted].any(), name          # every planted record is an outlier
        if exact:
            assert inl[~planted].all(), name
        else:
            outside += n_out
            rot, dr, _ = _pose_errors(m, pair, E, xa, xb, inl)
            noisy[pair] = [max(noisy[pair][0], rot), max(noisy[pair][1], dr)]
            line += ", rotation %.3f deg, direction %.3f deg" % (rot, dr)
        if planted.any():
            good = sum(1 for h in range(rc.H)
                       if not planted[list(rc.sample_np(rc.SEED, rc.pair_key(*pair), h, n))].any())
            fewest = min(fewest, good)
            line += ", all-inlier samples %d of %d" % (good, rc.H)
            assert good >= 8, name
        print(line)
    assert near == 0                                  # the cap on near-threshold records
    assert outside == rc.NOISY_INLIERS_OUTSIDE
    print("fewest all-inlier samples %d (written %d); noisy pose %s (written %s)" % (
        fewest, rc.MIN_ALL_INLIER_SAMPLES, noisy, rc.NOISY_POSE))
    assert rc.MIN_ALL_INLIER_SAMPLES <= fewest and rc.MIN_ALL_INLIER_SAMPLES >= 8
    for pair, (rot, dr) in noisy.items():
        assert rot <= rc.NOISY_POSE[pair][0] <= 4.0 * rot, pair
        assert dr <= rc.NOISY_POSE[pair][1] <= 4.0 * dr, pair


def test_hand_built_scenes():
    """The parallax gates of the device tests, from the ground truth: no record within PARALLAX_NEAR of a gate; the
    almost pure rotation stays below its written maximum, which is below its gate; the planar scene's eight-record
    samples have no determined null direction for numpy either."""
    par = rc.true_parallax(rc.base_scene("exact"), 4, 5)
    print("pair (4, 5): parallax %.3f .. %.3f deg, %d of %d at or above the gate" % (
        np.degrees(par.min()), np.degrees(par.max()), (par >= rc.PARALLAX_GATE).sum(), len(par)))
    assert (np.abs(par - rc.PARALLAX_GATE) > rc.PARALLAX_NEAR).all()
    assert 16 <= (par >= rc.PARALLAX_GATE).sum() <= len(par) - 16      # the gate splits the records
    m = rc.near_rotation_scene()
    assert abs(rc.true_rel(m, 4, 5)[2] - rc.NEAR_ROTATION_MM) < 1e-9
    worst = float(np.degrees(rc.true_parallax(m, 4, 5).max()))
    print("near rotation: largest parallax %.4f deg, written %.4f" % (worst, rc.NEAR_ROTATION_MAX_PARALLAX_DEG))
    assert worst <= rc.NEAR_ROTATION_MAX_PARALLAX_DEG <= 4.0 * worst
    assert np.radians(rc.NEAR_ROTATION_MAX_PARALLAX_DEG) < rc.NEAR_ROTATION_GATE - rc.PARALLAX_NEAR
    mp = rc.planar_scene()
    _, _, xa, xb, _, _ = rc.pair_records(mp, 4, 5)
    gaps = []
    for h in range(64):
        idx = list(rc.sample_np(rc.SEED, rc.pair_key(4, 5), h, len(xa)))
        w = rc.eight_point_np(xa[idx], xb[idx])[2]
        gaps.append((w[1] - w[0]) / w[8])
    print("planar: largest relative gap of 64 samples %.3e" % max(gaps))
    assert max(gaps) < 1e-12
