"""sg_slam_match_epipolar on the device against the numpy reference of epipolar_cases.py.

All five per-keypoint arrays and the per-pair counts are integers and must equal the reference exactly:
test_epipolar_reference_bounds.py holds every case clear of the only floating-point ambiguity (a decision within 1e-9
relative of its threshold).  The shapes case reaches every chunk, tile and slice boundary, so a padded tile entry that
counted would show in num_candidates there.  Also: a pair's answer does not depend on its position in the call or on
the run; the empty shapes; the map is not written; and, end to end, the accepted matches of a pair triangulate to the
scene's landmarks."""
import numpy as np
import pytest

import epipolar_cases as ec
import triangulate_cases as tc

pytestmark = pytest.mark.gpu

MAP_ARRAYS = ("q", "t", "k", "X", "obs_disabled", "point_flags")
NONE = (np.zeros((0, 2)), np.zeros((0, 4), dtype=np.uint64), np.zeros(0, dtype=np.int32))


@pytest.fixture(scope="module")
def slam():
    from slamgpu.ba import Slam
    return Slam(device=0)


def run(slam, c, sel=None, keypoints_a=None, keypoints_b=None):
    """The case's pairs (or those at the positions sel), with their own keypoints unless others are given."""
    sel = range(len(c.pairs)) if sel is None else sel
    ka, kb = ec.call_keypoints(c, "a"), ec.call_keypoints(c, "b")
    keypoints_a = [ka[i] for i in sel] if keypoints_a is None else keypoints_a
    keypoints_b = [kb[i] for i in sel] if keypoints_b is None else keypoints_b
    if not c.levels:
        keypoints_a, keypoints_b = [k[:2] for k in keypoints_a], [k[:2] for k in keypoints_b]
    before = {n: getattr(c.m, n).tobytes() for n in MAP_ARRAYS}
    counters = (slam.iterations(), slam.error())
    got = slam.MatchEpipolar(c.m, [c.pairs[i] for i in sel], keypoints_a, keypoints_b, **c.options)
    res = slam.epipolar_match_results()
    assert len(got) == len(res) == len(sel)
    assert all(np.array_equal(g, r["match"]) for g, r in zip(got, res))
    assert before == {n: getattr(c.m, n).tobytes() for n in before}, "the map was written"
    assert counters == (slam.iterations(), slam.error()), "the solver counters moved"
    return res


def same(a, b):
    return all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in ec.ARRAYS) and \
        all(a[k] == b[k] for k in ec.COUNTS)


def is_empty(r, na, nb, degenerate=0):
    return all((r[k] == -1).all() and len(r[k]) == na for k in ec.ARRAYS[:4]) and (r["num_candidates"] == 0).all() and \
        [r[k] for k in ec.COUNTS] == [na, nb, 0, 0, degenerate]


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_equals_the_reference_exactly(slam, name):
    c, want = ec.case(name), ec.expected(name)
    got = run(slam, c)
    for p, g, w in zip(c.pairs, got, want):
        print("%s pair %s: %s" % (name, p, {k: g[k] for k in ec.COUNTS}))
        for k in ec.COUNTS:
            assert g[k] == w[k], (name, p, k, g[k], w[k])
        for k in ec.ARRAYS:
            bad = np.flatnonzero(g[k] != w[k])
            assert len(bad) == 0, (name, p, k, len(bad), bad[:5], g[k][bad[:5]], w[k][bad[:5]])
            assert g[k].dtype == np.int32


def test_position_independence_and_reproducibility(slam):
    c = ec.case("c1_levels_parallax")     # four pairs
    first = run(slam, c)
    again = run(slam, c)
    assert all(same(a, b) for a, b in zip(first, again))
    rev = run(slam, c, sel=[3, 2, 1, 0])
    assert all(same(a, b) for a, b in zip(first, rev[::-1]))
    alone = run(slam, c, sel=[1])
    assert same(first[1], alone[0])
    # a pair listed twice, the second time with the head of its a keypoints: their rows are the same but for match,
    # which the missing claimants may change
    ka = ec.call_keypoints(c, "a")
    head = tuple(x[:50] for x in ka[0])
    twice = run(slam, c, sel=[0, 2, 0], keypoints_a=[ka[0], ka[2], head])
    assert same(twice[0], first[0]) and same(twice[1], first[2])
    assert all(np.array_equal(twice[2][k], first[0][k][:50]) for k in ec.ARRAYS if k != "match")
    # the shapes case: several slices per pair, merged in any order of the workgroups
    sh = ec.case("shapes")
    n = len(sh.pairs)
    a, b = run(slam, sh), run(slam, sh, sel=list(range(n))[::-1])
    assert all(same(x, y) for x, y in zip(a, b[::-1]))


def test_empty_shapes(slam):
    c = ec.case("c1_levels")
    ka, kb = ec.call_keypoints(c, "a"), ec.call_keypoints(c, "b")
    want = ec.expected("c1_levels")
    assert slam.MatchEpipolar(c.m, [], [], [], **c.options) == [] and slam.epipolar_match_results() == []   # n == 0
    # a pair without a keypoints and a pair without b keypoints between two full pairs
    got = run(slam, c, sel=[0, 1, 2, 3], keypoints_a=[ka[0], NONE, ka[2], ka[3]], keypoints_b=[kb[0], kb[1], NONE, kb[3]])
    assert is_empty(got[1], 0, len(kb[1][0])) and is_empty(got[2], len(ka[2][0]), 0)
    assert all(all(np.array_equal(got[i][k], want[i][k]) for k in ec.ARRAYS) for i in (0, 3))
    # every pair empty: nothing is launched (a handle that never matched answers too)
    from slamgpu.ba import Slam
    fresh = Slam(device=0)
    got = run(fresh, c, sel=[0, 1], keypoints_a=[NONE, ka[1]], keypoints_b=[kb[0], NONE])
    assert is_empty(got[0], 0, len(kb[0][0])) and is_empty(got[1], len(ka[1][0]), 0)


def test_accepted_matches_triangulate_to_the_landmarks(slam):
    """Detect -> Describe -> this call -> TriangulatePoints: the accepted true matches of pair (0, 1), appended to a
    copy of the map as new points with two observations each, come out at the scene's landmarks, within the bounds
    test_triangulate_gpu.py::test_exact_scenes holds the noise-free scenes to."""
    c = ec.case("c1")
    (fa, fb), t = c.pairs[0], c.truth[0]
    ka, kb = c.keypoints_a[0], c.keypoints_b[0]
    match = run(slam, c, sel=[0])[0]["match"]
    ok = match[t.ia] == t.jb
    ia, jb, landmark = t.ia[ok], t.jb[ok], t.point[ok]
    assert len(ia) >= 40
    m = c.m.copy()
    P0, n = m.num_points, len(ia)
    m.X = np.concatenate([m.X, np.tile([0.0, 0.0, 0.0, 1.0], n)])            # (the location at entry is not read)
    m.point_flags = np.concatenate([m.point_flags, np.zeros(n, dtype=np.int32)])
    m.point_uncertainty = np.concatenate([m.point_uncertainty, np.ones(n)])
    new = np.arange(P0, P0 + n, dtype=np.int32)
    m.obs_pt = np.concatenate([m.obs_pt, ka[0][ia].reshape(-1), kb[0][jb].reshape(-1)])
    m.obs_frame = np.concatenate([m.obs_frame, np.full(n, fa, dtype=np.int32), np.full(n, fb, dtype=np.int32)])
    m.obs_point = np.concatenate([m.obs_point, new, new])
    m.obs_disabled = np.concatenate([m.obs_disabled, np.zeros(2 * n, dtype=np.int32)])
    m.obs_error = np.concatenate([m.obs_error, np.zeros(4 * n)])
    solved = slam.TriangulatePoints(m, new)
    res = slam.triangulation_results()
    assert all(solved) and all(r["status"] == "OK" for r in res)
    truth = c.m.X_true.reshape(-1, 4)[landmark]
    dx = np.linalg.norm(m.X.reshape(-1, 4)[new] - truth, axis=1)
    gap = np.array([r["rel_gap"] for r in res])
    print("%d new points: worst |dX| %.2e, worst |dX| rel_gap %.2e" % (n, dx.max(), (dx * gap).max()))
    assert dx.max() <= tc.MARGIN * tc.SPREAD_X and (dx * gap).max() <= tc.MARGIN * tc.SPREAD_X_GAP
