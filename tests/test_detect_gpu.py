"""sg_tracker_detect / sg_frontend_detect on the device against the numpy reference (tests/detect_cases.py).  The device
detects on its own pyramid; the test downloads each level with sg_tracker_get_level, runs the reference on it and
demands exact equality of count, xy, levels, score and per_level, for every case and every option set
(tests/test_detect_reference_bounds.py shows that the cases hold what the equality is about).

Images: 161 x 121 at depth 3 (partial last cells), 96 x 64 with a padded row stride (its last level, 24 x 16, is one
partial cell), the planted squares on 97 x 70, a constant image, and 33 x 9 (one admissible row, an empty second cell
column, a second level too small for anything)."""
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc
from slamgpu.capi import SgDetectLevel
from slamgpu.tracker import default_detect_options, detect_cap
from slamgpu.video import SEQ_K as K, matcher_sequence, sequence_mark, sequence_pose, sequence_true_t

pytestmark = pytest.mark.gpu

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
EINVAL = -22
FIELDS = ("width", "height", "cells", "candidates", "low_cells", "keypoints")


@pytest.fixture(scope="module")
def trackers(gpu_lib):
    """One tracker per case with the case's image in slot 1, and the levels it built."""
    from slamgpu.tracker import HessianTracker
    out = {}
    for name in dc.CASES:
        c = dc.case(name)
        t = HessianTracker(window=13, depth=c.depth, max_images=3)
        assert t.lib.sg_tracker_set_image(t.h, 1, c.img.ctypes.data_as(C.POINTER(C.c_uint8)), c.w, c.h,
                                          c.img.strides[0]) == 0
        out[name] = (t, [t.level(1, l) for l in range(c.depth)])
    yield out
    for t, _ in out.values():
        t.close()


def _same(got, want, label=""):
    xy, lv, sc, per = got
    np.testing.assert_array_equal(xy, want.xy, err_msg=label + " xy")
    np.testing.assert_array_equal(lv, want.levels, err_msg=label + " levels")
    np.testing.assert_array_equal(sc.view(np.uint32), want.score.view(np.uint32), err_msg=label + " score")
    assert per == want.per_level, label


@pytest.mark.parametrize("name", dc.CASES)
def test_detect_equals_the_reference_on_the_device_pyramid(trackers, name):
    t, levels = trackers[name]
    total = 0
    for on, o in dc.option_sets(levels).items():
        want = dc.detect(levels, **o)
        got = t.Detect(1, **dict(dc.DEFAULTS, **o))
        _same(got, want, name + "/" + on)
        total += len(want.xy)
    assert t.detect_ms() > 0.0
    if name in dc.TEXTURE_CASES:
        assert total >= 300


def test_device_levels_are_the_oracle_levels(trackers, oracle_lib):
    """The CPU tests run on the oracle's pyramids: the same arrays as the device's."""
    for name in dc.CASES:
        for a, b in zip(trackers[name][1], dc.case_levels(name)):
            np.testing.assert_array_equal(a, b)


def test_two_runs_and_another_slot_give_the_same_bits(trackers):
    t, _ = trackers["odd"]
    c = dc.case("odd")
    a = t.Detect(1, **dc.DEFAULTS)
    b = t.Detect(1, **dc.DEFAULTS)
    t.MakePyramid(c.img, 2)
    d = t.Detect(2, **dc.DEFAULTS)
    assert len(a[0]) >= 50
    for x, y, z in zip(a, b, d):
        if isinstance(x, list):
            assert x == y == z
        else:
            assert x.tobytes() == y.tobytes() == z.tobytes()


def test_output_goes_straight_into_describe(trackers):
    t, _ = trackers["odd"]
    for opts in (dict(border=15), dict(border=20, per_cell=16)):
        xy, lv, sc, _ = t.Detect(1, **dict(dc.DEFAULTS, **opts))
        assert len(xy) >= 50 and len(set(lv)) >= 2
        on_level = xy.astype(np.float64) / (2.0 ** lv)[:, None]
        assert (on_level == np.rint(on_level)).all()
        desc, ang, st = t.Describe(1, xy, lv)
        assert (st == 0).all() and (ang >= 0).all()
    # border 4 keypoints are too close to the edge for some descriptors: DetectAndDescribe returns the others
    xy, lv, sc, _ = t.Detect(1, **dc.DEFAULTS)
    st = t.Describe(1, xy, lv)[2]
    assert (st == 1).any() and (st == 0).any()
    kx, kl, ks, desc, ang = t.DetectAndDescribe(1, **dc.DEFAULTS)
    np.testing.assert_array_equal(kx, xy[st == 0])
    np.testing.assert_array_equal(kl, lv[st == 0])
    np.testing.assert_array_equal(ks, sc[st == 0])
    np.testing.assert_array_equal(desc, t.Describe(1, xy, lv)[0][st == 0])
    assert len(ang) == len(kx) and (ang >= 0).all()


class _Call:
    """Raw sg_tracker_detect arguments over sentinel-filled arrays."""

    def __init__(self, t, n, depth, **opts):
        self.lib, self.h, self.n = t.lib, t.h, n
        self.o = default_detect_options(**dict(dc.DEFAULTS, **opts))
        self.xy = np.full((n, 2), -7.0, np.float32)
        self.lv = np.full(n, -8, np.int32)
        self.sc = np.full(n, -9.0, np.float32)
        self.count = C.c_int32(-10)
        self.per = (SgDetectLevel * depth)()
        for p in self.per:
            p.width = -11
        self.args = dict(h=self.h, slot=1, o=C.byref(self.o), cap=n, xy=self.xy.ctypes.data_as(_fp),
                         lv=self.lv.ctypes.data_as(_ip), sc=self.sc.ctypes.data_as(_fp), count=C.byref(self.count),
                         per=self.per)

    def __call__(self, fn=None, **kw):
        a = dict(self.args, **kw)
        return (fn or self.lib.sg_tracker_detect)(a["h"], a["slot"], a["o"], a["cap"], a["xy"], a["lv"], a["sc"],
                                                  a["count"], a["per"])

    def untouched(self):
        return ((self.xy == -7.0).all() and (self.lv == -8).all() and (self.sc == -9.0).all() and
                self.count.value == -10 and all(p.width == -11 for p in self.per))

    def per_level(self):
        return [p.as_dict() for p in self.per]


def test_cap_below_count_writes_the_first_and_leaves_the_rest(trackers):
    t, levels = trackers["odd"]
    want = dc.detect(levels)
    n = len(want.xy)
    assert n >= 50
    k = 37
    call = _Call(t, n, 3)
    assert call(cap=k) == 0
    assert call.count.value == n
    np.testing.assert_array_equal(call.xy[:k], want.xy[:k])
    np.testing.assert_array_equal(call.lv[:k], want.levels[:k])
    np.testing.assert_array_equal(call.sc[:k], want.score[:k])
    assert (call.xy[k:] == -7.0).all() and (call.lv[k:] == -8).all() and (call.sc[k:] == -9.0).all()
    assert call.per_level() == want.per_level      # the record counts every keypoint, written or not
    # cap == 0 with null arrays returns the count
    call = _Call(t, n, 3)
    assert call(cap=0, xy=None, lv=None, sc=None, per=None) == 0
    assert call.count.value == n and (call.xy == -7.0).all()
    # score and per_level may be null
    call = _Call(t, n, 3)
    assert call(sc=None, per=None) == 0
    assert call.count.value == n and (call.sc == -9.0).all() and call.per[0].width == -11
    np.testing.assert_array_equal(call.xy, want.xy)
    np.testing.assert_array_equal(call.lv, want.levels)
    # the wrapper's capacity is the bound the contract names
    assert detect_cap(161, 121, 3, 4) == (24 + 6 + 2) * 4


def test_every_einval_leaves_the_outputs_untouched(trackers):
    t, levels = trackers["odd"]
    n = len(dc.detect(levels).xy)
    call = _Call(t, n, 3)

    def opt(**kw):
        return C.byref(default_detect_options(**dict(dc.DEFAULTS, **kw)))
    cases = dict(
        null_handle=dict(h=None), null_options=dict(o=None), null_count=dict(count=None), negative_cap=dict(cap=-1),
        null_xy=dict(xy=None), null_levels=dict(lv=None), slot_low=dict(slot=-1), slot_high=dict(slot=3),
        slot_never_set=dict(slot=0), first_level_low=dict(o=opt(first_level=-1)), first_level_high=dict(o=opt(first_level=3)),
        num_levels_negative=dict(o=opt(num_levels=-1)), range_past_depth=dict(o=opt(first_level=1, num_levels=3)),
        threshold_nan=dict(o=opt(threshold=float("nan"))), threshold_inf=dict(o=opt(threshold=float("inf"))),
        min_threshold_nan=dict(o=opt(min_threshold=float("nan"))), min_threshold_negative=dict(o=opt(min_threshold=-0.001)),
        thresholds_crossed=dict(o=opt(min_threshold=0.5, threshold=0.25)),
        border_low=dict(o=opt(border=3)), border_high=dict(o=opt(border=65)), per_cell_low=dict(o=opt(per_cell=0)),
        per_cell_high=dict(o=opt(per_cell=17)), max_keypoints_negative=dict(o=opt(max_keypoints=-1)))
    for name, kw in cases.items():
        assert call(**kw) == EINVAL, name
        assert call.untouched(), name
    ms = C.c_double(5.0)
    assert t.lib.sg_tracker_detect_ms(None, C.byref(ms)) == EINVAL and ms.value == 5.0
    assert t.lib.sg_tracker_detect_ms(t.h, None) == EINVAL
    # the extremes of every range are accepted, and so are the same arguments, unbroken
    for kw in (dict(border=64), dict(border=4, per_cell=16), dict(first_level=2, num_levels=1), dict(min_threshold=0.0),
               dict(min_threshold=-0.0, threshold=0.0), dict(first_level=1, num_levels=2)):
        assert call(o=opt(**kw)) == 0, kw
    assert call() == 0 and call.count.value == n and (call.lv >= 0).all()


# ------------------------------------------------------------------------------------------------ the front end
def _empty_map():
    from slamgpu.scene import MapArrays
    z = lambda dt: np.zeros(0, dt)  # noqa: E731
    return MapArrays(k=K.copy(), q=z(np.float64), t=z(np.float64), frame_camera=z(np.int32), frame_prev=z(np.int32),
                     X=z(np.float64), point_flags=z(np.int32), point_uncertainty=z(np.float64), obs_pt=z(np.float64),
                     obs_frame=z(np.int32), obs_point=z(np.int32), obs_disabled=z(np.int32), obs_error=z(np.float64),
                     frame_keyframe=z(np.int32))


DETECT_OPTS = dict(dc.DEFAULTS, border=15, num_levels=3)


def _run_sequence(frames, detect=False):
    """Matcher::Track over the frames as tests/test_frontend.py drives it: (per-frame stats, observations, what
    Detect gave for every held keyframe view after every frame when `detect` is set)."""
    from slamgpu.frontend import Matcher, add_frame
    m = _empty_map()
    mt = Matcher(window=13, depth=6)
    stats, detected = [], {}
    for i, img in enumerate(frames):
        q, t = sequence_pose(i)
        add_frame(m, 0, q, t)
        sequence_mark(i, m.point_flags, m.point_uncertainty, m.num_points)

        def upd(i=i):
            m.t[3 * i:3 * i + 3] = sequence_true_t(i)
            return i % 2 == 1
        assert mt.Track(img, i, 0, m, upd)
        stats.append(dict(mt.last_stats))
        if detect:
            held = [f for f in range(i + 1) if m.frame_keyframe[f]][-4:]
            for f in held:      # every held view, the older ones again and again
                detected[(i, f)] = mt.Detect(f, **DETECT_OPTS)
    obs = (m.obs_pt.copy(), m.obs_frame.copy(), m.obs_point.copy(), m.X.copy())
    mt.close()
    return stats, obs, detected, m.frame_keyframe.copy()


def test_frontend_detect_equals_the_tracker_and_leaves_tracking_alone(gpu_lib):
    from slamgpu.frontend import Matcher, add_frame
    from slamgpu.tracker import HessianTracker
    sequence = matcher_sequence()[0]
    plain_stats, plain_obs, _, _ = _run_sequence(sequence)
    stats, obs, detected, keyframe = _run_sequence(sequence, True)
    assert stats == plain_stats
    for a, b in zip(obs, plain_obs):
        np.testing.assert_array_equal(a, b)
    assert sum(keyframe) >= 3 and len(detected) > sum(keyframe)
    t = HessianTracker(window=13, depth=6, max_images=2)
    for (i, f), got in detected.items():
        t.MakePyramid(sequence[f], 1)
        want = t.Detect(1, **DETECT_OPTS)
        assert len(want[0]) >= 50 and len(want[3]) == 6 and want[3][3]["cells"] == 0
        for g, w in zip(got, want):
            if isinstance(g, list):
                assert g == w
            else:
                np.testing.assert_array_equal(g, w, err_msg="frame %d detected after frame %d" % (f, i))
    t.close()
    # a frame with no view: any frame of a fresh front end, one that never became a keyframe, one out of range
    mt = Matcher(window=13, depth=6)
    o = default_detect_options(**DETECT_OPTS)
    count = C.c_int32(-10)
    args = (C.byref(o), 0, None, None, None, C.byref(count), None)
    assert mt.lib.sg_frontend_detect(mt.h, 0, *args) == EINVAL
    assert mt.lib.sg_frontend_detect(None, 0, *args) == EINVAL
    m = _empty_map()
    for i in (0, 1):
        add_frame(m, 0, *sequence_pose(i))
        assert mt.Track(sequence[i], i, 0, m)
    assert m.frame_keyframe[0] == 1 and m.frame_keyframe[1] == 0
    assert mt.lib.sg_frontend_detect(mt.h, 1, *args) == EINVAL      # tracked, but not kept as a view
    assert mt.lib.sg_frontend_detect(mt.h, 99, *args) == EINVAL
    assert mt.lib.sg_frontend_detect(mt.h, 0, None, *args[1:]) == EINVAL and count.value == -10
    assert mt.lib.sg_frontend_detect(mt.h, 0, *args) == 0 and count.value >= 50
    with pytest.raises(Exception):
        mt.Detect(1)
    mt.close()
