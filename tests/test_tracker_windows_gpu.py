"""The device tracker (csrc/tracker.hip, csrc/corners.hip) against the oracle at every window size, on odd image sizes
and on deep pyramids (the cases of tracker_cases.py; tests/test_tracker_cases.py holds them to their conditions).

Every comparison is assert_array_equal: the device follows the oracle operation for operation, so positions,
acceptance flags, status and Newton iteration counts are the same bits or the kernel is wrong.

Which test runs which instantiation (NK = ceil(W^2 / 64)):
  k_track_fb<1>       test_fb_tracking_bit_exact[a_w2, a_w8]
  k_track_fb<2>       test_fb_tracking_bit_exact[a_w9 .. a_w11, b_*_w9], test_device_resident_path[9], test_batch_edges
  k_track_fb<3>       test_fb_tracking_bit_exact[a_w12, b_*_w13]
  k_track_fb<4>       test_fb_tracking_bit_exact[a_w14 .. a_w16, b_*_w16], test_device_resident_path[16]
  k_track_one<2>, <4> test_track_feature_hessian[9], [16]
  k_find_matches<2>, <4>  test_matcher_windows[9], [16]
  k_track_klt, k_brute_* (not instantiated per NK) at W = 8, 10, 16: test_track_feature_klt, test_track_feature_brute
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import tracker_cases as tc
from slamgpu.tracker import HessianTracker
from slamgpu.video import SEQ_K, make_frames, matcher_sequence, seed_points, sequence_mark, sequence_pose, sequence_true_t

pytestmark = pytest.mark.gpu

HESSIAN, KLT, BRUTE = 0, 1, 2
_u8p = C.POINTER(C.c_uint8)
_device_fb = {}   # case name -> the device's TrackFeatureFB result (shared by the tests that compare with it)


@pytest.fixture(scope="module", autouse=True)
def _libs(gpu_lib, oracle_lib):
    return gpu_lib


def _tracker(c, **kw):
    t = HessianTracker(window=c.window, depth=c.depth, retry_levels=c.retry_levels, **kw)
    t.MakePyramid(c.frames[0], 0)
    t.MakePyramid(c.frames[1], 1)
    return t


def device_fb(name):
    if name not in _device_fb:
        c = tc.case(name)
        t = _tracker(c)
        _device_fb[name] = t.TrackFeatureFB(0, 1, c.pts, c.start, c.levels)
        t.close()
    return _device_fb[name]


@pytest.mark.parametrize("name", tc.CASE_NAMES)
def test_fb_tracking_bit_exact(name):
    c = tc.case(name)
    if name in tc.B_NAMES:   # the pyramid first: odd sizes at every depth, down to 3 x 2 at depth 8
        t = _tracker(c)
        for slot, flat in enumerate(tc.pyramids(c.w, c.h, c.depth)[:2]):
            for l, ref in enumerate(oracle.pyramid_levels(flat, tc.pyramids(c.w, c.h, c.depth)[2])):
                np.testing.assert_array_equal(t.level(slot, l), ref, err_msg="slot %d level %d" % (slot, l))
        t.close()
    out, acc, its = device_fb(name)
    ro, racc, rits = tc.expected(name)
    np.testing.assert_array_equal(acc.astype(np.int32), racc)
    np.testing.assert_array_equal(its, rits)
    np.testing.assert_array_equal(out, ro)


@pytest.mark.parametrize("W", [9, 16])
def test_device_resident_path(W):
    """load_features / run / results (the benchmark's path) gives what TrackFeatureFB gives, repeats included."""
    name = "a_w%d" % W
    c = tc.case(name)
    t = _tracker(c)
    t.load_features(c.pts, c.start, c.levels)
    t.run(0, 1, repeats=2)
    out, acc, its = t.results()
    t.close()
    fo, facc, fits = device_fb(name)
    np.testing.assert_array_equal(acc, facc)
    np.testing.assert_array_equal(its, fits)
    np.testing.assert_array_equal(out, fo)


@pytest.mark.parametrize("n", [1, 5, 7])
def test_batch_edges(n):
    """A feature's answer does not depend on its wave or workgroup: the first n features alone (a partial last
    workgroup of kTrackWaves = 4) give the first n rows of the full run."""
    c = tc.case("a_w9")
    t = _tracker(c)
    out, acc, its = t.TrackFeatureFB(0, 1, c.pts[:n], c.start[:n], c.levels[:n])
    t.close()
    fo, facc, fits = device_fb("a_w9")
    np.testing.assert_array_equal(acc, facc[:n])
    np.testing.assert_array_equal(its, fits[:n])
    np.testing.assert_array_equal(out, fo[:n])


# ------------------------------------------------------------------------------------- one-directional TrackFeature
@pytest.fixture(scope="module")
def frames():
    return tc.frames(640, 480)


def _track_feature(frames, mode, W, depth, pts, start, levels=None):
    t = HessianTracker(window=W, depth=depth, mode=mode)
    t.MakePyramid(frames[0], 0)
    t.MakePyramid(frames[1], 1)
    got = t.TrackFeature(0, 1, pts, start, levels)
    t.close()
    pf, dims = oracle.make_pyramid_mode(frames[0], depth, mode)
    pt, _ = oracle.make_pyramid_mode(frames[1], depth, mode)
    ref = oracle.track_feature_mode(mode, pf, pt, dims, W, pts, start, levels=levels, nthreads=tc.NTHREADS)
    (go, gs, gi), (ro, rs, ri) = got, ref
    np.testing.assert_array_equal(gs, rs)
    np.testing.assert_array_equal(gi, ri)
    np.testing.assert_array_equal(go, ro)
    return rs


@pytest.mark.parametrize("W", [9, 16])
def test_track_feature_hessian(frames, W):
    """k_track_one<2> and <4>: HessianTracker::TrackFeature alone, 3 and 6 levels mixed."""
    rng = np.random.default_rng(W)
    pts = seed_points(100)
    start = (pts + rng.normal(0, 0.4, pts.shape)).astype(np.float32)
    levels = np.where(rng.random(len(pts)) < 0.3, 6, 3).astype(np.int32)
    st = _track_feature(frames, HESSIAN, W, 6, pts, start, levels)
    assert (st == 0).mean() >= 0.95   # (the oracle's: 99 - 100 %)


@pytest.mark.parametrize("W", [8, 10, 16])
def test_track_feature_klt(frames, W):
    rng = np.random.default_rng(W)
    pts = seed_points(64)
    start = (pts + rng.normal(0, 0.4, pts.shape)).astype(np.float32)
    st = _track_feature(frames, KLT, W, 3, pts, start)
    assert (st == 0).all()


@pytest.mark.parametrize("W", [8, 16])
def test_track_feature_brute(frames, W):
    """Three interior points and three inside brute.h's 13 px margin (status 2)."""
    rng = np.random.default_rng(W)
    pts = np.array([[200.5, 150.25], [420, 300], [333.3, 222.2], [6, 200], [630.5, 40], [100, 470]], np.float32)
    start = (pts + rng.normal(0, 0.4, pts.shape)).astype(np.float32)
    st = _track_feature(frames, BRUTE, W, 3, pts, start)
    assert st.tolist() == [0, 0, 0, 2, 2, 2]


# ------------------------------------------------------------------------------------------------ k_find_matches
MATCHER_LOG = {   # the oracle's (matches_first, matches, keyframe, added) on the first six frames
    9: [(0, 0, 1, 120), (106, 106, 0, 0), (105, 105, 0, 0), (10, 17, 1, 103), (98, 98, 0, 0), (10, 14, 1, 104)],
    16: [(0, 0, 1, 120), (109, 109, 0, 0), (105, 105, 0, 0), (12, 16, 1, 105), (101, 101, 0, 0), (8, 14, 1, 106)],
}


@pytest.mark.parametrize("W", [9, 16])
def test_matcher_windows(W):
    """k_find_matches<2> and <4>: Matcher::Track with a 9 and a 16 pixel window over the first six frames of the
    matcher sequence (seeding, plain tracking, a cut keyframe, the re-match after update_frames) against the
    sequential oracle matcher with the same window."""
    from slamgpu.frontend import Matcher, add_frame
    from slamgpu.scene import MapArrays
    frames = matcher_sequence()[0][:6]
    omap, omt, olog = tc.run_oracle(frames, window=W)
    assert [(s["matches_first"], s["matches"], s["keyframe"], s["added"]) for s in olog] == MATCHER_LOG[W]
    z = lambda dt: np.zeros(0, dt)  # noqa: E731
    m = MapArrays(k=SEQ_K.copy(), q=z(np.float64), t=z(np.float64), frame_camera=z(np.int32), frame_prev=z(np.int32),
                  X=z(np.float64), point_flags=z(np.int32), point_uncertainty=z(np.float64), obs_pt=z(np.float64),
                  obs_frame=z(np.int32), obs_point=z(np.int32), obs_disabled=z(np.int32), obs_error=z(np.float64),
                  frame_keyframe=z(np.int32))
    mt = Matcher(window=W, depth=6)
    for i, img in enumerate(frames):
        q, t = sequence_pose(i)
        add_frame(m, 0, q, t)
        sequence_mark(i, m.point_flags, m.point_uncertainty, m.num_points)

        def upd(i=i):
            m.t[3 * i:3 * i + 3] = sequence_true_t(i)
            return i % 2 == 1
        assert mt.Track(img, i, 0, m, upd)
        st = mt.last_stats
        for key in ("matches_first", "matches", "keyframe", "corners", "added", "features", "views"):
            assert st[key] == olog[i][key], (i, key, st[key], olog[i][key])
        got = [(float(m.obs_pt[2 * o]), float(m.obs_pt[2 * o + 1]), int(m.obs_point[o]))
               for o in np.nonzero(m.obs_frame == i)[0]]
        assert got == omap.obs[i], "frame %d observations differ" % i
    assert m.num_points == len(omap.X)
    np.testing.assert_array_equal(m.point_flags, np.array(omap.flags))
    np.testing.assert_array_equal(m.frame_keyframe, np.array(omap.keyframe))
    pts, ids = mt.features()
    assert list(ids) == sorted(omt.features) and list(pts) == [omt.features[f]["point"] for f in sorted(omt.features)]
    mt.close()


# ------------------------------------------------------------------------------------------------ row stride
def _set_image(t, slot, view):
    h, w = view.shape[:2]
    rc = t.lib.sg_tracker_set_image(t.h, slot, C.cast(view.ctypes.data, _u8p), w, h, view.strides[0])
    assert rc == 0


@pytest.mark.parametrize("mode", [HESSIAN, KLT])
@pytest.mark.parametrize("w,h", [(211, 97), (640, 480)])
def test_row_stride(w, h, mode):
    """A cv::Mat-style view into a wider image (stride > 3 w, the last row ending with the allocation) gives the
    pyramid and the corners of its contiguous copy, whatever the bytes between the rows are.  (An over-read past the
    last row is not observable here; sg_tracker_set_image's contract in include/slamgpu.h excludes it.)"""
    rng = np.random.default_rng(w + mode)
    parent = rng.integers(0, 256, (h, w + 19, 3), dtype=np.uint8)
    view = parent[:, 19:, :]
    assert view.strides[0] == 3 * (w + 19) and not view.flags["C_CONTIGUOUS"]
    assert view.ctypes.data + view.strides[0] * (h - 1) + 3 * w == parent.ctypes.data + parent.nbytes
    depth = 6
    t = HessianTracker(window=13, depth=depth, mode=mode)
    t.MakePyramid(view.copy(), 0)
    want = [t.level(0, l) for l in range(depth)]
    want_c = t.SeedFeatures(0)
    for fill in (None, 0, 255):
        if fill is not None:
            parent[:, :19, :] = fill
        _set_image(t, 1, view)
        for l in range(depth):
            np.testing.assert_array_equal(t.level(1, l), want[l], err_msg="level %d, padding %s" % (l, fill))
        got_c = t.SeedFeatures(1)
        np.testing.assert_array_equal(got_c[0], want_c[0])
        np.testing.assert_array_equal(got_c[1], want_c[1])
    assert len(want_c[0]) > 0
    t.close()


# ------------------------------------------------------------------------------------------------ corner seeding
SEED_PARAMS = [(120, 20.0), (1024, 1.0), (1024, 3.0), (7, 5.0)]   # (max_corners, min_distance)
SEED_COUNTS = {   # the oracle's corner counts per parameter set: the kMaxSeed cap and the uncapped side both occur
    (211, 97): (40, 870, 751, 7),
    (321, 241): (120, 1024, 1024, 7),
    (160, 163): (47, 1024, 979, 7),
    (33, 31): (3, 32, 27, 7),
}


@pytest.mark.parametrize("w,h", list(SEED_COUNTS))
def test_seed_features_off_640x480(w, h):
    img = make_frames(1, w, h)[0]
    t = HessianTracker(window=13, depth=3)
    t.MakePyramid(img, 0)
    counts = []
    for max_corners, min_distance in SEED_PARAMS:
        kw = dict(max_corners=max_corners, min_distance=min_distance)
        co, ao = oracle.seed_features(img, None, **kw)
        cg, ag = t.SeedFeatures(0, None, **kw)
        np.testing.assert_array_equal(cg, co)
        np.testing.assert_array_equal(ag, ao)
        matches = co[::4] + 0.5
        co2, ao2 = oracle.seed_features(img, matches, **kw)
        cg2, ag2 = t.SeedFeatures(0, matches, **kw)
        np.testing.assert_array_equal(cg2, co2)
        np.testing.assert_array_equal(ag2, ao2)
        assert len(ao2) < len(co2)
        counts.append(len(co))
    t.close()
    assert tuple(counts) == SEED_COUNTS[(w, h)]
