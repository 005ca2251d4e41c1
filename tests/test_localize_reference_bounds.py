"""The bounds of the localization tests, from the references alone (numpy and the CPU oracle; no GPU, no library):

  * SPREAD_EXACT_PX: on the exact scenes, the worst reprojection error over a frame's records at p3p_newton_np's pose
    from one fixed, well-spread sample per frame (spread_sample: the records nearest to three image positions far
    apart), over the test frames.  The device is held to MARGIN = 100 times it.
  * At the oracle's pose-only optimum started from the truth, on every case the GPU tests check a mask on: no record
    within NEAR = 1e-6 px of TAU (cap 0, so an inlier mask is not a matter of rounding); every planted outlier is an
    outlier there; every other record is an inlier on the exact scenes, and on the noisy ones the count that is not
    is NOISY_INLIERS_OUTSIDE.
  * kPnpMinW excludes no record of these scenes."""
import numpy as np

import localize_cases as lc


def test_spread_exact_px_is_the_reference_error():
    worst = 0.0
    m = lc.base_scene("exact")
    for f in lc.FRAMES:
        _, pt, X, k = lc.frame_records(m, f)
        q_true, t_true = lc.true_pose(m, f)
        idx = lc.spread_sample(pt)
        P = X[idx, :3] / X[idx, 3:4]
        q, t = lc.p3p_newton_np(lc.bearings_np(k, pt[idx]), P, np.linalg.norm(P - t_true, axis=1))
        e, inl, _ = lc.score_np(q, t, k, X, pt)
        print("frame %d: sample %s, worst error %.3e px, q off %.3e, t off %.3e" % (
            f, idx, e.max(), np.abs(q - q_true).max(), np.abs(t - t_true).max()))
        assert inl.all()
        worst = max(worst, float(e.max()))
    print("recomputed %.3e px, written %.3e px" % (worst, lc.SPREAD_EXACT_PX))
    assert worst <= lc.SPREAD_EXACT_PX <= 4.0 * worst
    assert lc.MARGIN == 100.0


def test_no_record_near_the_threshold_and_the_planted_mask_is_the_inlier_mask(oracle_lib):
    near = outside = 0
    for name, m, f, planted, exact in lc.all_cases():
        s, q, t = lc.oracle_pose(oracle_lib, m, f, *lc.true_pose(m, f))
        assert s["ok"] == 1, name
        _, pt, X, k = lc.frame_records(m, f)
        assert len(planted) == len(pt)
        e, inl, _ = lc.score_np(q, t, k, X, pt)
        n_near = int((np.abs(e - lc.TAU) <= lc.NEAR).sum())
        n_out = int((~inl & ~planted).sum())
        print("%s: N %d, planted %d, near %d, unplanted outside %d, smallest planted error %.2f px, largest other "
              "%.3e px" % (name, len(pt), planted.sum(), n_near, n_out,
                           e[planted].min() if planted.any() else np.inf, e[~planted].max()))
        near += n_near
        assert not inl[planted].any(), name          # every planted outlier is an outlier
        if exact:
            assert inl[~planted].all(), name
        else:
            outside += n_out
        assert (np.abs(X[:, 3]) >= lc.PNP_MIN_W).all(), name
    assert near == 0                                  # the cap on near-threshold records
    assert outside == lc.NOISY_INLIERS_OUTSIDE
