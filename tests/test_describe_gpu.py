"""sg_tracker_describe / sg_frontend_describe on the device against the numpy reference (tests/describe_cases.py).  The
device describes from its own pyramid; the test downloads each level with sg_tracker_get_level, runs the reference on
it and demands exact equality of desc, angle_bin and status (every accepted keypoint of the cases has a gap of 1e-9
or more: tests/test_describe_reference_bounds.py).

Images: 161 x 121 at depth 3 (levels 161 x 121, 81 x 61 and 41 x 31, which leaves only the row cy = 15) and 96 x 64
with a padded row stride (its last level, 24 x 16, refuses everything).  Calls of 1, 3, 4, 5 and 257 keypoints: a lone
wave, a partial workgroup, a full one, one plus a wave, many.  Keypoints on every border side of every level and one
pixel inside, coordinates ending in .5, NaN and infinite coordinates, levels = NULL."""
import ctypes as C

import numpy as np
import pytest

import describe_cases as dc
from slamgpu.video import SEQ_K as K, matcher_sequence, sequence_mark, sequence_pose, sequence_true_t

pytestmark = pytest.mark.gpu

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint64)
EINVAL = -22


@pytest.fixture(scope="module")
def trackers(gpu_lib):
    """One tracker per device case with the case's image in slot 1, and the levels it built."""
    from slamgpu.tracker import HessianTracker
    out = {}
    for name in dc.DEVICE_CASES:
        c = dc.device_case(name)
        t = HessianTracker(window=13, depth=c.depth, max_images=3)
        check = t.lib.sg_tracker_set_image(t.h, 1, c.img.ctypes.data_as(C.POINTER(C.c_uint8)), c.w, c.h, c.img.strides[0])
        assert check == 0
        out[name] = (t, [t.level(1, l) for l in range(c.depth)])
    yield out
    for t, _ in out.values():
        t.close()


def _same(got, want, n=None):
    for key, g in zip(("desc", "angle_bin", "status"), got):
        np.testing.assert_array_equal(g, want[key][:n], err_msg=key)


@pytest.mark.parametrize("name", list(dc.DEVICE_CASES))
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257])
def test_describe_equals_the_reference_on_the_device_pyramid(trackers, name, n):
    t, levels = trackers[name]
    c = dc.device_case(name)
    want = dc.reference(levels, c.xy, c.levels)
    ok = want["status"] == 0
    assert (want["gap"][ok] >= dc.GAP).all()
    got = t.Describe(1, c.xy[:n], c.levels[:n])
    _same(got, want, n)
    if n == dc.N_DEVICE:
        assert ok.sum() >= 100 and (~ok).sum() >= 30 and t.describe_ms() > 0.0
        assert (got[1][~ok] == -1).all() and not got[0][~ok].any()


@pytest.mark.parametrize("name", list(dc.DEVICE_CASES))
def test_null_levels_means_level_0(trackers, name):
    t, levels = trackers[name]
    c = dc.device_case(name)
    want = dc.reference(levels, c.xy, None)
    assert (want["gap"][want["status"] == 0] >= dc.GAP).all() and (want["status"] == 0).sum() > 50
    _same(t.Describe(1, c.xy, None), want)


def test_two_runs_and_a_reversed_order_give_the_same_bits(trackers):
    t, _ = trackers["odd"]
    c = dc.device_case("odd")
    a = t.Describe(1, c.xy, c.levels)
    b = t.Describe(1, c.xy, c.levels)
    r = t.Describe(1, c.xy[::-1], c.levels[::-1])
    for x, y, z in zip(a, b, r):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z[::-1])


def test_optional_outputs_may_be_null(trackers):
    t, _ = trackers["odd"]
    c = dc.device_case("odd")
    full = t.Describe(1, c.xy, c.levels)
    desc = np.zeros((dc.N_DEVICE, 4), np.uint64)
    xy = np.ascontiguousarray(c.xy)
    lv = np.ascontiguousarray(c.levels)
    assert t.lib.sg_tracker_describe(t.h, 1, dc.N_DEVICE, xy.ctypes.data_as(_fp), lv.ctypes.data_as(_ip),
                                     desc.ctypes.data_as(_up), None, None) == 0
    np.testing.assert_array_equal(desc, full[0])


def test_zero_keypoints_launch_nothing(trackers):
    t, _ = trackers["odd"]
    c = dc.device_case("odd")
    t.Describe(1, c.xy[:5], c.levels[:5])
    ms = t.describe_ms()
    assert ms > 0.0
    desc, ang, st = t.Describe(1, np.zeros((0, 2), np.float32))
    assert desc.shape == (0, 4) and len(ang) == 0 and len(st) == 0
    assert t.lib.sg_tracker_describe(t.h, 1, 0, None, None, None, None, None) == 0
    assert t.describe_ms() == ms      # the last launch is still the one before


def test_every_einval_leaves_the_outputs_untouched(trackers):
    t, _ = trackers["odd"]
    c = dc.device_case("odd")
    lib = t.lib
    n = 6
    xy = np.ascontiguousarray(c.xy[:n])
    lv = np.ascontiguousarray(c.levels[:n])
    desc = np.full((n, 4), 0xABCDABCDABCDABCD, np.uint64)
    ang = np.full(n, 77, np.int32)
    st = np.full(n, 78, np.int32)
    p = dict(h=t.h, slot=1, n=n, xy=xy.ctypes.data_as(_fp), lv=lv.ctypes.data_as(_ip), desc=desc.ctypes.data_as(_up))

    def call(**kw):
        a = dict(p, **kw)
        return lib.sg_tracker_describe(a["h"], a["slot"], a["n"], a["xy"], a["lv"], a["desc"], ang.ctypes.data_as(_ip),
                                       st.ctypes.data_as(_ip))
    bad_hi = lv.copy()
    bad_hi[n - 1] = c.depth
    bad_lo = lv.copy()
    bad_lo[0] = -1
    cases = dict(null_handle=dict(h=None), negative_n=dict(n=-1), null_xy=dict(xy=None), null_desc=dict(desc=None),
                 slot_low=dict(slot=-1), slot_high=dict(slot=3), slot_never_set=dict(slot=0),
                 level_high=dict(lv=bad_hi.ctypes.data_as(_ip)), level_negative=dict(lv=bad_lo.ctypes.data_as(_ip)),
                 too_many=dict(n=(1 << 20) + 1))
    for name, kw in cases.items():
        assert call(**kw) == EINVAL, name
        assert (desc == 0xABCDABCDABCDABCD).all() and (ang == 77).all() and (st == 78).all(), name
    assert lib.sg_tracker_describe(t.h, 0, 0, None, None, None, None, None) == EINVAL      # the slot rule holds at n = 0
    ms = C.c_double(5.0)
    assert lib.sg_tracker_describe_ms(None, C.byref(ms)) == EINVAL and ms.value == 5.0
    assert call() == 0 and (st != 78).all()      # and the same arguments, unbroken, are accepted


# ------------------------------------------------------------------------------------------------ the front end
def _empty_map():
    from slamgpu.scene import MapArrays
    z = lambda dt: np.zeros(0, dt)  # noqa: E731
    return MapArrays(k=K.copy(), q=z(np.float64), t=z(np.float64), frame_camera=z(np.int32), frame_prev=z(np.int32),
                     X=z(np.float64), point_flags=z(np.int32), point_uncertainty=z(np.float64), obs_pt=z(np.float64),
                     obs_frame=z(np.int32), obs_point=z(np.int32), obs_disabled=z(np.int32), obs_error=z(np.float64),
                     frame_keyframe=z(np.int32))


def _run_sequence(frames, describe_xy=None):
    """Matcher::Track over the frames as tests/test_frontend.py drives it: (per-frame stats, observations, per-frame
    descriptors of held keyframe views when describe_xy is given)."""
    from slamgpu.frontend import Matcher, add_frame
    m = _empty_map()
    mt = Matcher(window=13, depth=6)
    stats, described = [], {}
    for i, img in enumerate(frames):
        q, t = sequence_pose(i)
        add_frame(m, 0, q, t)
        sequence_mark(i, m.point_flags, m.point_uncertainty, m.num_points)

        def upd(i=i):
            m.t[3 * i:3 * i + 3] = sequence_true_t(i)
            return i % 2 == 1
        assert mt.Track(img, i, 0, m, upd)
        stats.append(dict(mt.last_stats))
        if describe_xy is not None:
            held = [f for f in range(i + 1) if m.frame_keyframe[f]][-4:]
            for f in held:      # every held view, the older ones again and again
                described[(i, f)] = mt.Describe(f, describe_xy, np.arange(len(describe_xy)) % 3)
    obs = (m.obs_pt.copy(), m.obs_frame.copy(), m.obs_point.copy(), m.X.copy())
    mt.close()
    return stats, obs, described, m.frame_keyframe.copy()


@pytest.fixture(scope="module")
def sequence():
    return matcher_sequence()[0]      # all of it: more than four keyframes, so views expire between describe calls


def test_frontend_describe_equals_the_tracker_and_leaves_tracking_alone(gpu_lib, sequence):
    from slamgpu.frontend import Matcher
    from slamgpu.tracker import HessianTracker
    from slamgpu.video import SEQ_H, SEQ_W, seed_points
    xy = seed_points(90, SEQ_W, SEQ_H, border=12.0)
    plain_stats, plain_obs, _, _ = _run_sequence(sequence)
    stats, obs, described, keyframe = _run_sequence(sequence, xy)
    assert stats == plain_stats
    for a, b in zip(obs, plain_obs):
        np.testing.assert_array_equal(a, b)
    assert sum(keyframe) >= 3 and len(described) > sum(keyframe)
    lv = np.arange(len(xy)) % 3
    t = HessianTracker(window=13, depth=6, max_images=2)
    for (i, f), got in described.items():
        t.MakePyramid(sequence[f], 1)
        want = t.Describe(1, xy, lv)
        assert (want[2] == 0).sum() > 40 and (want[2] == 1).sum() > 0
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w, err_msg="frame %d described after frame %d" % (f, i))
    t.close()
    # a frame with no view: one that never became a keyframe, one out of range, and any frame of a fresh front end
    mt = Matcher(window=13, depth=6)
    desc = np.full((2, 4), 9, np.uint64)
    args = (2, xy[:2].ctypes.data_as(_fp), None, desc.ctypes.data_as(_up), None, None)
    assert mt.lib.sg_frontend_describe(mt.h, 0, *args) == EINVAL
    assert mt.lib.sg_frontend_describe(None, 0, *args) == EINVAL
    m = _empty_map()
    from slamgpu.frontend import add_frame
    for i in (0, 1):
        add_frame(m, 0, *sequence_pose(i))
        assert mt.Track(sequence[i], i, 0, m)
    assert m.frame_keyframe[0] == 1 and m.frame_keyframe[1] == 0
    assert mt.lib.sg_frontend_describe(mt.h, 0, *args) == 0 and (desc != 9).any()
    desc[:] = 9
    assert mt.lib.sg_frontend_describe(mt.h, 1, *args) == EINVAL      # tracked, but not kept as a view
    assert mt.lib.sg_frontend_describe(mt.h, 99, *args) == EINVAL
    assert (desc == 9).all()
    with pytest.raises(Exception):
        mt.Describe(1, xy[:2])
    mt.close()
