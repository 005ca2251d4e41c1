"""The bounds of the landmark-alignment tests, from the numpy references of tests/align_cases.py alone (no GPU, no
library):

  * COUNT_C1 and LONG_COUNT: the record counts.
  * SPREAD_EXACT: on the exact cases, the rotation, translation and log-scale errors and the worst residual of the
    reference Horn from one fixed well-spread sample of three records (spread_sample), worst over the cases.  The code
    under test is held to MARGIN = 100 times these values.  The log scale of an exact case is often exactly 0 in numpy,
    so its floor is one unit of fp64 rounding, EPS.
  * At the reference's all-inlier estimate from the non-planted records, on every case a mask is checked on: no record
    within NEAR = 1e-6 of TAU (cap 0); every planted record an outlier; every other record an inlier, on the noisy
    scenes too (cap 0: the noise is TAU / 8 per coordinate).
  * For each case with planted wrong matches, the all-inlier samples among the H hypotheses of seed SEED, counted
    with the numpy sampler, are at least 8 and at least MIN_ALL_INLIER_SAMPLES.
  * NOISY_POSE: the all-inlier estimate's errors against the truth on the noisy cases.
  * The hand-built scenes' gaps against the gates of the device tests.
A written constant must be an upper bound, and within a factor of 4 of the recomputed value."""
import numpy as np

import align_cases as ac

EPS = 2.220446049250313e-16
KEYS = ("rot_deg", "t", "log_scale")


def test_record_counts():
    m, corr, _ = ac.scene("exact", 0.0)
    ok, X, _ = ac.records(m, corr)
    assert ok.all() and len(X) == ac.COUNT_C1 == len(corr)
    m, corr, _ = ac.long_scene(0.0)
    ok, X, _ = ac.records(m, corr)
    assert ok.all() and len(X) == ac.LONG_COUNT > 1024
    assert max(ac.COUNTS) < ac.COUNT_C1


def test_spread_exact_is_the_reference_error():
    worst = {"rot_deg": 0.0, "t": 0.0, "log_scale": EPS, "resid": 0.0}
    for name, m, corr, planted, noise, kind in ac.all_cases():
        if noise != "exact":
            continue
        _, X, Y = ac.records(m, corr)
        keep = np.flatnonzero(~planted)
        idx = keep[ac.spread_sample(X[keep])]
        s, R, t, gap = ac.horn_np(X[idx], Y[idx], kind == "rigid")
        e, inl, _ = ac.score_np(s, R, t, X, Y)
        err = ac.errors(s, R, t, kind)
        print("%s: sample %s, gap %.3f, rotation %.3e deg, translation %.3e, log scale %.3e, worst residual %.3e" % (
            name, list(idx), gap, *err, e[~planted].max()))
        assert gap > 100 * ac.MIN_GAP and np.array_equal(inl, ~planted)
        for key, v in zip(KEYS + ("resid",), err + (float(e[~planted].max()),)):
            worst[key] = max(worst[key], v)
    print("recomputed %s, written %s" % (worst, ac.SPREAD_EXACT))
    for key, v in worst.items():
        assert v <= ac.SPREAD_EXACT[key] <= 4.0 * v, key
    assert ac.MARGIN == 100.0


def test_masks_thresholds_sample_counts_and_noisy_pose():
    near = 0
    fewest = ac.H
    noisy = dict.fromkeys(KEYS, 0.0)
    for name, m, corr, planted, noise, kind in ac.all_cases():
        ok, X, Y = ac.records(m, corr)
        n = len(X)
        assert ok.all() and len(planted) == n, name
        s, R, t, gap = ac.horn_np(X[~planted], Y[~planted], kind == "rigid")
        e, inl, _ = ac.score_np(s, R, t, X, Y)
        n_near = int((np.abs(e - ac.TAU) <= ac.NEAR).sum())
        near += n_near
        line = "%s: N %d, planted %d, near %d, gap %.3f, smallest planted residual %.1f, largest other %.3e" % (
            name, n, planted.sum(), n_near, gap, e[planted].min() if planted.any() else np.inf, e[~planted].max())
        assert not inl[planted].any(), name          # every planted record is an outlier
        assert inl[~planted].all(), name             # every other record is an inlier, on the noisy scenes too
        assert gap > 100 * ac.MIN_GAP, name
        if noise == "noisy":
            err = ac.errors(s, R, t, kind)
            for key, v in zip(KEYS, err):
                noisy[key] = max(noisy[key], v)
            line += ", rotation %.3e deg, translation %.3e, log scale %.3e" % err
        if planted.any():
            key = int(corr[0, 0])
            good = sum(1 for h in range(ac.H) if not planted[list(ac.sample_np(ac.SEED, key, h, n))].any())
            fewest = min(fewest, good)
            line += ", all-inlier samples %d of %d" % (good, ac.H)
            assert good >= 8, name
        print(line)
    assert near == 0                                  # the cap on near-threshold records
    print("fewest all-inlier samples %d (written %d); noisy pose %s (written %s)" % (
        fewest, ac.MIN_ALL_INLIER_SAMPLES, noisy, ac.NOISY_POSE))
    assert 8 <= ac.MIN_ALL_INLIER_SAMPLES <= fewest
    for key, v in noisy.items():
        assert v <= ac.NOISY_POSE[key] <= 4.0 * v, key


def test_planted_records_are_far():
    m, corr, planted = ac.scene("exact", ac.SHARE)
    _, X, Y = ac.records(m, corr)
    d = np.linalg.norm(Y - ac.apply_true(X), axis=1)
    assert planted.sum() == round(ac.SHARE * len(X))
    assert (d[planted] >= 10 * ac.TAU - 1e-6).all() and (d[~planted] < 1e-9).all()


def test_hand_built_scenes():
    gaps = {}
    for name in ("collinear", "thin", "planar", "mirror", "random"):
        m, corr = getattr(ac, name + "_scene")()
        ok, X, Y = ac.records(m, corr)
        assert ok.all()
        s, R, t, gaps[name] = ac.horn_np(X, Y)
        _, inl, _ = ac.score_np(s, R, t, X, Y)
        print("%s: N %d, gap %.3e, scale %.4f, inliers of the all-record fit %d" % (name, len(X), gaps[name], s,
                                                                                  inl.sum()))
        if name in ("mirror", "random"):
            assert inl.sum() < 8          # no similarity joins the two sides
            # the best of the H three-record hypotheses.  Mirrored: the sample itself (a triangle and its mirror image
            # are congruent) and the few landmarks near its plane.  Random: not even the sample, whose two triangles
            # are not similar.
            key, n = int(corr[0, 0]), len(X)
            most = 0
            for h in range(ac.H):
                idx = list(ac.sample_np(ac.SEED, key, h, n))
                sh, Rh, th, gh = ac.horn_np(X[idx], Y[idx])
                if gh > 1e-12:
                    most = max(most, int(ac.score_np(sh, Rh, th, X, Y)[1].sum()))
            print("%s: most inliers of a hypothesis %d of %d" % (name, most, n))
            assert (most >= 3 if name == "mirror" else most < 3) and most < n // (4 * ac.HAND_MIN_INLIERS_SHARE)
        else:
            assert inl.all()
    assert gaps["collinear"] < 1e-12
    assert 1e-12 < gaps["thin"] < ac.MIN_GAP / 100
    for name in ("planar", "mirror", "random"):
        assert gaps[name] > 100 * ac.MIN_GAP
    # the thin scene still gives models: its three-record samples keep a gap above the solver's 1e-12
    m, corr = ac.thin_scene()
    _, X, Y = ac.records(m, corr)
    g = [ac.horn_np(X[list(i)], Y[list(i)])[3]
         for i in (ac.sample_np(ac.SEED, int(corr[0, 0]), h, len(X)) for h in range(256))]
    print("thin: three-record gaps %.3e .. %.3e" % (min(g), max(g)))
    assert sum(v > 1e-11 for v in g) >= 8
