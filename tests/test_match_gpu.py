"""sg_slam_match_by_projection on the device against the numpy reference of match_cases.py.

All five per-keypoint arrays and the per-frame counts are integers and must equal the reference exactly:
test_match_reference_bounds.py holds every case clear of the only floating-point ambiguity (a distance at the radius,
a projection at an image border or at the behind-camera line).  Also: the window search with a radius beyond the image
equals the all-pairs sg_hamming_match; a frame's answer does not depend on its position in the call or on the run;
the empty shapes."""
import numpy as np
import pytest

import match_cases as mc

pytestmark = pytest.mark.gpu

ARRAYS = ("match", "best_point", "best_dist", "second_dist", "num_candidates")
COUNTS = ("num_keypoints", "num_projected", "num_with_candidates", "num_matched")


@pytest.fixture(scope="module")
def slam():
    from slamgpu.ba import Slam
    return Slam(device=0)


def run(slam, c, frames=None, keypoints=None, **opt):
    o = dict(c.options)
    o.update(opt)
    frames = c.frames if frames is None else frames
    keypoints = c.keypoints if keypoints is None else keypoints
    before = {n: getattr(c.m, n).tobytes() for n in ("q", "t", "k", "X", "obs_disabled", "point_flags")}
    got = slam.MatchByProjection(c.m, frames, keypoints, c.points, c.point_desc, radius_px=o["radius_px"],
                                 max_dist=o["max_dist"], ratio_percent=o["ratio_percent"],
                                 skip_observed=bool(o["skip_observed"]), width=o["width"], height=o["height"])
    res = slam.projection_match_results()
    assert len(got) == len(res) == len(frames)
    assert all(np.array_equal(g, r["match"]) for g, r in zip(got, res))
    assert before == {n: getattr(c.m, n).tobytes() for n in before}, "the map was written"
    return res


def same(a, b):
    return all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in ARRAYS) and \
        all(a[k] == b[k] for k in COUNTS)


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_equals_the_reference_exactly(slam, name):
    c, want = mc.case(name), mc.expected(name)
    got = run(slam, c)
    for f, g, w in zip(c.frames, got, want):
        print("%s frame %d: %s" % (name, f, {k: g[k] for k in COUNTS}))
        for k in COUNTS:
            assert g[k] == w[k], (name, f, k, g[k], w[k])
        for k in ARRAYS:
            bad = np.flatnonzero(g[k] != w[k])
            assert len(bad) == 0, (name, f, k, len(bad), bad[:5], g[k][bad[:5]], w[k][bad[:5]])
            assert g[k].dtype == np.int32


def test_a_wide_radius_equals_the_all_pairs_matcher(slam):
    from slamgpu.matcher import HammingMatcher
    c = mc.case("c1_skip_off")
    # beyond the image diagonal of every projection: all points in front of frame 3 are in every window
    got = run(slam, c, frames=[3], keypoints=[c.keypoints[0]], radius_px=1e5)[0]
    assert got["num_projected"] == len(c.points) and (got["num_candidates"] == len(c.points)).all()
    hm = HammingMatcher(device=0)
    bi, bd, sd = hm.match(c.keypoints[0][1], c.point_desc)
    hm.close()
    assert np.array_equal(got["best_point"], c.points[bi])
    assert np.array_equal(got["best_dist"], bd) and np.array_equal(got["second_dist"], sd)


def test_position_independence_and_reproducibility(slam):
    c = mc.case("c1_bounded")        # three frames
    first = run(slam, c)
    again = run(slam, c)
    assert all(same(a, b) for a, b in zip(first, again))
    rev = run(slam, c, frames=c.frames[::-1], keypoints=c.keypoints[::-1])
    assert all(same(a, b) for a, b in zip(first, rev[::-1]))
    alone = run(slam, c, frames=c.frames[1:2], keypoints=c.keypoints[1:2])
    assert same(first[1], alone[0])
    # a frame listed twice, each time with its own keypoints
    head = (c.keypoints[0][0][:50], c.keypoints[0][1][:50])
    twice = run(slam, c, frames=[c.frames[0], c.frames[2], c.frames[0]],
                keypoints=[c.keypoints[0], c.keypoints[2], head])
    assert same(twice[0], first[0]) and same(twice[1], first[2])
    assert all(np.array_equal(twice[2][k], first[0][k][:50]) for k in ARRAYS if k != "match")
    # the long case too: its survivor lists are compacted by many waves in any order
    lg = mc.case("long")
    a, b = run(slam, lg), run(slam, lg, frames=lg.frames[::-1], keypoints=lg.keypoints[::-1])
    assert all(same(x, y) for x, y in zip(a, b[::-1]))


def test_empty_shapes(slam):
    c = mc.case("planted_skip_on")
    none = (np.zeros((0, 2)), np.zeros((0, 4), dtype=np.uint64))
    got = run(slam, c, frames=[4, 7], keypoints=[none, none])                       # K == 0
    assert all(len(g["match"]) == 0 and [g[k] for k in COUNTS] == [0, 0, 0, 0] for g in got)
    nopoints = mc.SimpleNamespace(m=c.m, frames=c.frames, keypoints=c.keypoints, points=np.zeros(0, dtype=np.int32),
                                  point_desc=np.zeros((0, 4), dtype=np.uint64), options=c.options)
    got = run(slam, nopoints)                                                       # np == 0
    for g, kp in zip(got, c.keypoints):
        assert all((g[k] == -1).all() for k in ARRAYS[:4]) and (g["num_candidates"] == 0).all()
        assert [g[k] for k in COUNTS] == [len(kp[0]), 0, 0, 0]
    assert slam.MatchByProjection(c.m, [], [], c.points, c.point_desc) == []        # n == 0
