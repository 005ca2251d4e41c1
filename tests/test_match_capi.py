"""Argument handling of sg_slam_match_by_projection, its option defaults and struct layouts: needs the library but no
GPU.  (Every argument error is found by the host-only planner before the device is touched.)"""
import ctypes as C

import numpy as np

import match_cases as mc
from slamgpu.capi import SgMatchOptions, SgMatchResult, load_library

IP, DP, UP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
MAP_ARRAYS = ("k", "q", "t", "X", "point_flags", "point_uncertainty", "obs_pt", "obs_frame", "obs_point",
              "obs_disabled", "obs_error", "frame_camera", "frame_prev")


def _options(lib):
    o = SgMatchOptions(radius_px=7.0, width=7, height=7, max_dist=7, ratio_percent=7, skip_observed=7)
    lib.sg_match_options_default(C.byref(o))
    return o


def test_symbols_defaults_and_struct_layouts():
    lib = load_library()
    assert lib.sg_slam_match_by_projection and lib.sg_match_options_default
    o = _options(lib)
    assert (o.radius_px, o.width, o.height, o.max_dist, o.ratio_percent, o.skip_observed) == (12.0, 0, 0, 64, 80, 1)
    # the C layouts: a double and five 32-bit fields, padded to a multiple of 8 | four ints
    assert C.sizeof(SgMatchOptions) == 32 and C.sizeof(SgMatchResult) == 16
    assert [getattr(SgMatchOptions, n).offset for n, _ in SgMatchOptions._fields_] == [0, 8, 12, 16, 20, 24]
    assert [getattr(SgMatchResult, n).offset for n, _ in SgMatchResult._fields_] == [0, 4, 8, 12]


def test_argument_errors_return_before_the_device_is_touched():
    lib = load_library()
    f = lib.sg_slam_match_by_projection
    c = mc.case("planted_skip_on")
    m = c.m.copy()
    before = {n: getattr(m, n).tobytes() for n in MAP_ARRAYS}
    ms = m.struct()
    buf = C.create_string_buffer(64)
    dummy = C.cast(buf, C.c_void_p)   # an opaque non-null handle: it must never be touched
    raw = bytes(buf.raw)
    frames = np.array(c.frames, dtype=np.int32)
    off = np.zeros(len(frames) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(k[0]) for k in c.keypoints])
    K = int(off[-1])
    xy = np.concatenate([k[0] for k in c.keypoints]).reshape(-1)
    kd = np.concatenate([k[1] for k in c.keypoints]).reshape(-1)
    pts = np.ascontiguousarray(c.points, dtype=np.int32)
    pd = np.ascontiguousarray(c.point_desc, dtype=np.uint64).reshape(-1)
    outs = [np.full(K, 7, dtype=np.int32) for _ in range(5)]
    res = (SgMatchResult * len(frames))()
    res[0].num_projected = 77
    good = dict(handle=dummy, mp=C.byref(ms), frames=frames, n=len(frames), off=off, xy=xy, kd=kd, pts=pts, np=len(pts),
                pd=pd, match=outs[0])

    def call(opt, **kw):
        a = dict(good)
        a.update(kw)
        p = lambda v, t: None if v is None else v.ctypes.data_as(t)   # noqa: E731
        return f(a["handle"], a["mp"], p(a["frames"], IP), a["n"], p(a["off"], IP), p(a["xy"], DP), p(a["kd"], UP),
                 p(a["pts"], IP), a["np"], p(a["pd"], UP), opt, p(a["match"], IP), *[p(x, IP) for x in outs[1:]], res)

    o = C.byref(_options(lib))
    for kw in (dict(handle=None), dict(mp=None), dict(match=None), dict(n=-1), dict(np=-1), dict(frames=None),
               dict(off=None), dict(xy=None), dict(kd=None), dict(pts=None), dict(pd=None)):
        assert call(o, **kw) == -22, kw
    assert call(None) == -22
    assert call(None, n=0) == -22                                      # null options, even with n == 0
    assert call(o, match=None, n=0) == -22
    bad = off.copy()
    bad[0] = 1
    assert call(o, off=bad) == -22
    bad = off.copy()
    bad[1] = bad[2] + 1
    assert call(o, off=bad) == -22
    assert call(o, off=np.array([0, 2 ** 20 + 1], dtype=np.int32), n=1) == -22
    for v in (-1, m.num_frames, 2 ** 31 - 1):
        b = frames.copy()
        b[1] = v
        assert call(o, frames=b) == -22, v
    for v in (-1, m.num_points, 2 ** 31 - 1):
        b = pts.copy()
        b[3] = v
        assert call(o, pts=b) == -22, v
    b = pts.copy()
    b[5] = b[2]
    assert call(o, pts=b) == -22                                       # a point listed twice
    for field, v in (("radius_px", 0.0), ("radius_px", -12.0), ("radius_px", float("nan")), ("radius_px", float("inf")),
                     ("width", -1), ("height", -1), ("width", 640), ("height", 480), ("max_dist", -1), ("max_dist", 257),
                     ("ratio_percent", 0), ("ratio_percent", 101)):
        b = _options(lib)
        setattr(b, field, v)
        assert call(C.byref(b)) == -22, (field, v)
        assert call(C.byref(b), n=0) == -22, (field, v)
    # n * np above 2^22: one frame listed 2^22 / np + 1 times (the keypoint arrays are then not read)
    many = 2 ** 22 // len(pts) + 1
    assert call(o, frames=np.full(many, 4, dtype=np.int32), n=many, off=np.zeros(many + 1, dtype=np.int32)) == -22
    # maps that cannot be read
    for name in ("q", "t", "k", "frame_camera", "X", "obs_frame", "obs_point", "obs_disabled"):
        broken = m.struct()
        setattr(broken, name, None)
        assert call(o, mp=C.byref(broken)) == -22, name
    m2 = m.copy()
    m2.obs_point[10] = m.num_points
    ms2 = m2.struct()
    assert call(o, mp=C.byref(ms2)) == -22                             # an observation index out of range
    m2 = m.copy()
    m2.frame_camera[4] = 2
    ms2 = m2.struct()
    assert call(o, mp=C.byref(ms2)) == -22                             # a camera index out of range
    assert lib.sg_last_error()
    assert call(o, n=0) == 0                                           # n == 0: a no-op, without a device
    assert call(o, n=0, frames=None, off=None, xy=None, kd=None, pts=None, pd=None) == 0
    # a failing call writes nothing: the map, the handle and every output are as they were
    assert all((x == 7).all() for x in outs) and res[0].num_projected == 77 and bytes(buf.raw) == raw
    assert {n: getattr(m, n).tobytes() for n in MAP_ARRAYS} == before


def test_empty_shapes_need_no_device():
    """K == 0 or np == 0: nothing is launched, so the answer comes without the handle being touched."""
    lib = load_library()
    f = lib.sg_slam_match_by_projection
    c = mc.case("planted_skip_on")
    ms = c.m.struct()
    buf = C.create_string_buffer(64)
    dummy, raw = C.cast(buf, C.c_void_p), bytes(buf.raw)
    o = _options(lib)
    frames = np.array([4, 2], dtype=np.int32)
    pts = np.ascontiguousarray(c.points, dtype=np.int32)
    pd = np.ascontiguousarray(c.point_desc, dtype=np.uint64).reshape(-1)
    res = (SgMatchResult * 2)()
    # K == 0
    off = np.zeros(3, dtype=np.int32)
    match = np.full(1, 7, dtype=np.int32)
    assert f(dummy, C.byref(ms), frames.ctypes.data_as(IP), 2, off.ctypes.data_as(IP), None, None,
             pts.ctypes.data_as(IP), len(pts), pd.ctypes.data_as(UP), C.byref(o), match.ctypes.data_as(IP), None, None,
             None, None, res) == 0
    assert match[0] == 7 and all((r.num_keypoints, r.num_projected, r.num_with_candidates, r.num_matched) == (0, 0, 0, 0)
                                 for r in res)
    # np == 0
    xy, kd = c.keypoints[0]
    K = len(xy)
    off = np.array([0, K, K], dtype=np.int32)
    outs = [np.full(K, 7, dtype=np.int32) for _ in range(5)]
    xy, kd = np.ascontiguousarray(xy).reshape(-1), np.ascontiguousarray(kd).reshape(-1)
    assert f(dummy, C.byref(ms), frames.ctypes.data_as(IP), 2, off.ctypes.data_as(IP), xy.ctypes.data_as(DP),
             kd.ctypes.data_as(UP), None, 0, None, C.byref(o), *[x.ctypes.data_as(IP) for x in outs], res) == 0
    assert all((x == -1).all() for x in outs[:4]) and (outs[4] == 0).all()
    assert [(r.num_keypoints, r.num_projected, r.num_with_candidates, r.num_matched) for r in res] == \
        [(K, 0, 0, 0), (0, 0, 0, 0)]
    assert bytes(buf.raw) == raw
