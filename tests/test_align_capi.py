"""Argument handling of sg_slam_align_points, its option defaults and struct sizes, and sg_map_apply_similarity (host
only): needs the library but no GPU.  (Every argument error is found by the host-only planner before the device is
touched.)"""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import localize_cases as lc
from slamgpu.capi import ALIGN_STATUS, SgAlignOptions, SgAlignResult, load_library
from slamgpu.scene import quat_from_matrix, quat_to_matrix

IP, DP = C.POINTER(C.c_int32), C.POINTER(C.c_double)
MAP_ARRAYS = ("k", "q", "t", "X", "point_flags", "point_uncertainty", "obs_pt", "obs_frame", "obs_point",
              "obs_disabled", "obs_error", "frame_camera", "frame_prev")


def _options(lib):
    o = SgAlignOptions(threshold=7.0, max_hypotheses=7, min_inliers=7, seed=7, refine=7, fix_scale=7, max_scale=7.0,
                       min_gap=7.0)
    lib.sg_align_options_default(C.byref(o))
    return o


def _arrays(m):
    return {n: getattr(m, n).tobytes() for n in MAP_ARRAYS}


def test_symbols_defaults_and_struct_sizes():
    lib = load_library()
    assert lib.sg_slam_align_points and lib.sg_align_options_default and lib.sg_map_apply_similarity
    o = _options(lib)
    assert (o.threshold, o.max_hypotheses, o.min_inliers, o.seed, o.refine, o.fix_scale, o.max_scale, o.min_gap) == \
        (10.0, 1024, 8, 0, 1, 0, 0.0, 1e-6)
    # the C sizes: a double, five 32-bit fields, padding, two doubles | eleven ints, padding, twelve doubles
    assert C.sizeof(SgAlignOptions) == 48 and C.sizeof(SgAlignResult) == 144
    assert SgAlignResult.msac_cost.offset == 48 and SgAlignResult.scale.offset == 80
    assert SgAlignOptions.max_scale.offset == 32
    assert ALIGN_STATUS == {0: "OK", 1: "DID_NOT_RUN", 2: "NO_MODEL", 3: "FEW_INLIERS", 4: "DEGENERATE"}


def test_argument_errors_return_before_the_device_is_touched():
    lib = load_library()
    f = lib.sg_slam_align_points
    m, corr, _ = ac.scene("exact", 0.0, count=8)
    before = _arrays(m)
    ms = m.struct()
    buf = C.create_string_buffer(64)
    dummy = C.cast(buf, C.c_void_p)   # an opaque non-null handle: it must never be touched
    raw = bytes(buf.raw)
    cr = np.ascontiguousarray(corr, dtype=np.int32).reshape(-1)
    off = np.array([0, len(corr)], dtype=np.int32)
    solved = (C.c_int32 * 1)(7)
    res = (SgAlignResult * 1)()
    res[0].status = 77
    inl = np.full(len(corr), 7, dtype=np.int32)

    def call(handle, mp, c, g, n, o, sv=solved):
        return f(handle, mp, None if c is None else c.ctypes.data_as(IP), None if g is None else g.ctypes.data_as(IP), n,
                 o, sv, res, inl.ctypes.data_as(IP))

    o = _options(lib)
    assert call(None, C.byref(ms), cr, off, 1, C.byref(o)) == -22
    assert call(dummy, None, cr, off, 1, C.byref(o)) == -22
    assert call(dummy, C.byref(ms), cr, off, 1, None) == -22
    assert call(dummy, C.byref(ms), None, None, 0, None) == -22          # null options, even with n == 0
    assert call(dummy, C.byref(ms), None, off, 1, C.byref(o)) == -22
    assert call(dummy, C.byref(ms), cr, None, 1, C.byref(o)) == -22
    assert call(dummy, C.byref(ms), cr, off, 1, C.byref(o), sv=None) == -22
    assert call(dummy, C.byref(ms), cr, off, -1, C.byref(o)) == -22
    assert call(dummy, C.byref(ms), cr, np.array([1, 8], dtype=np.int32), 1, C.byref(o)) == -22
    assert call(dummy, C.byref(ms), cr, np.array([0, 5, 4], dtype=np.int32), 2, C.byref(o)) == -22
    for bad in (-1, m.num_points, 2 ** 31 - 1):
        for side in (0, 1):
            c2 = cr.copy()
            c2[2 * 3 + side] = bad
            assert call(dummy, C.byref(ms), c2, off, 1, C.byref(o)) == -22, (bad, side)
    c2 = cr.copy()
    c2[5] = c2[4]
    assert call(dummy, C.byref(ms), c2, off, 1, C.byref(o)) == -22                      # a == b
    for field, bad in (("threshold", 0.0), ("threshold", -1.0), ("threshold", float("nan")), ("max_hypotheses", 0),
                       ("max_hypotheses", -256), ("min_gap", -1e-9), ("min_gap", float("nan")), ("max_scale", 0.5),
                       ("max_scale", -1.0), ("max_scale", float("nan"))):
        b = _options(lib)
        setattr(b, field, bad)
        assert call(dummy, C.byref(ms), cr, off, 1, C.byref(b)) == -22, (field, bad)
        assert call(dummy, C.byref(ms), None, None, 0, C.byref(b)) == -22, (field, bad)
    assert lib.sg_last_error()
    assert call(dummy, C.byref(ms), None, None, 0, C.byref(o)) == 0      # n == 0: a no-op, without a device
    assert call(dummy, C.byref(ms), cr, off, 0, C.byref(o)) == 0
    # a failing call writes nothing: the map, the handle and every output are as they were
    assert solved[0] == 7 and res[0].status == 77 and (inl == 7).all() and bytes(buf.raw) == raw
    assert _arrays(m) == before


# ------------------------------------------------------------------------------------ sg_map_apply_similarity
def _apply(lib, m, s, q, t, frames, points):
    ms = m.struct()
    qq, tt = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(t, dtype=np.float64)
    fr, pt = np.ascontiguousarray(frames, dtype=np.int32), np.ascontiguousarray(points, dtype=np.int32)
    return lib.sg_map_apply_similarity(C.byref(ms), s, qq.ctypes.data_as(DP), tt.ctypes.data_as(DP),
                                       fr.ctypes.data_as(IP), len(fr), pt.ctypes.data_as(IP), len(pt))


def _pixels(m, obs):
    """The numpy projection (localize_cases.project_np_q) of the listed observations at the map's poses and points."""
    out = np.zeros((len(obs), 2))
    for j, o in enumerate(obs):
        f, p = m.obs_frame[o], m.obs_point[o]
        k = m.k[7 * m.frame_camera[f]:7 * m.frame_camera[f] + 7]
        uv, ok = lc.project_np_q(m.q[4 * f:4 * f + 4], m.t[3 * f:3 * f + 3], k, m.X.reshape(-1, 4)[[p]])
        assert ok.all()
        out[j] = uv[0]
    return out


def test_apply_similarity_keeps_pixels_inverts_and_leaves_the_rest():
    lib = load_library()
    base = lc.base_scene("exact")
    frames = np.arange(5, 10, dtype=np.int32)
    seen = np.isin(base.obs_frame, frames)
    points = np.unique(base.obs_point[seen]).astype(np.int32)
    # observations of listed frames: all their points are listed, so every pixel must stay
    obs = np.flatnonzero(seen)[::7]
    s, q, t = ac.SCALES["sim"], quat_from_matrix(ac.R_TRUE), ac.T_TRUE
    m = base.copy()
    assert _apply(lib, m, s, q, t, frames, points) == 0
    px = np.abs(_pixels(m, obs) - _pixels(base, obs)).max()
    print("pixels of %d observations move by %.3e px" % (len(obs), px))
    assert px <= 1e-9
    # the numpy restatement of the transform
    want = ac.numpy_apply(base, s, ac.R_TRUE, t, frames, points)
    assert np.allclose(m.X, want.X, rtol=1e-13, atol=0) and np.allclose(m.t, want.t, rtol=1e-13, atol=1e-10)
    assert np.abs(m.q - want.q).max() < 1e-14
    qs = m.q.reshape(-1, 4)
    assert (np.abs(np.linalg.norm(qs, axis=1) - 1.0) < 1e-14).all() and (qs[:, 3] >= 0).all()
    assert np.array_equal(m.X.reshape(-1, 4)[points, 3], base.X.reshape(-1, 4)[points, 3])      # W stays: not renormalised
    # unlisted frames and points are bit-identical, and so is everything else of the map
    rest_f = np.setdiff1d(np.arange(base.num_frames), frames)
    rest_p = np.setdiff1d(np.arange(base.num_points), points)
    assert len(rest_f) and len(rest_p)
    assert np.array_equal(m.q.reshape(-1, 4)[rest_f], base.q.reshape(-1, 4)[rest_f])
    assert np.array_equal(m.t.reshape(-1, 3)[rest_f], base.t.reshape(-1, 3)[rest_f])
    assert np.array_equal(m.X.reshape(-1, 4)[rest_p], base.X.reshape(-1, 4)[rest_p])
    skip = ("q", "t", "X")
    assert {k: v for k, v in _arrays(m).items() if k not in skip} == \
        {k: v for k, v in _arrays(base).items() if k not in skip}
    # S, then the inverse of S: X = R^T (Y - t) / s
    Ri = ac.R_TRUE.T
    assert _apply(lib, m, 1.0 / s, quat_from_matrix(Ri), -Ri @ t / s, frames, points) == 0
    rel = max(np.abs(m.X - base.X).max() / np.abs(base.X).max(), np.abs(m.t - base.t).max() / np.abs(base.t).max(),
              np.abs(m.q - base.q).max())
    print("S then its inverse: off by %.3e relative" % rel)
    assert rel <= 1e-9
    # -q is the same rotation
    m1, m2 = base.copy(), base.copy()
    assert _apply(lib, m1, s, q, t, frames, points) == 0 and _apply(lib, m2, s, -q, t, frames, points) == 0
    assert np.array_equal(m1.X, m2.X) and np.array_equal(m1.t, m2.t) and np.array_equal(m1.q, m2.q)
    assert abs(np.linalg.det(quat_to_matrix(q)) - 1.0) < 1e-14


def test_apply_similarity_argument_errors_write_nothing():
    lib = load_library()
    m = lc.base_scene("exact")
    before = _arrays(m)
    q, t = quat_from_matrix(ac.R_TRUE), ac.T_TRUE
    ms = m.struct()
    fr, pt = np.array([5, 6], dtype=np.int32), np.array([1, 2, 3], dtype=np.int32)
    f = lib.sg_map_apply_similarity
    args = (1.3, q.ctypes.data_as(DP), t.ctypes.data_as(DP), fr.ctypes.data_as(IP), 2, pt.ctypes.data_as(IP), 3)
    assert f(None, *args) == -22
    assert f(C.byref(ms), 1.3, None, t.ctypes.data_as(DP), fr.ctypes.data_as(IP), 2, pt.ctypes.data_as(IP), 3) == -22
    assert f(C.byref(ms), 1.3, q.ctypes.data_as(DP), None, fr.ctypes.data_as(IP), 2, pt.ctypes.data_as(IP), 3) == -22
    assert f(C.byref(ms), 1.3, q.ctypes.data_as(DP), t.ctypes.data_as(DP), None, 2, pt.ctypes.data_as(IP), 3) == -22
    assert f(C.byref(ms), 1.3, q.ctypes.data_as(DP), t.ctypes.data_as(DP), fr.ctypes.data_as(IP), 2, None, 3) == -22
    assert f(C.byref(ms), 1.3, q.ctypes.data_as(DP), t.ctypes.data_as(DP), fr.ctypes.data_as(IP), -1, None, 0) == -22
    for bad_q in (2.0 * q, np.zeros(4), q * (1 + 1e-6), np.array([np.nan, 0, 0, 1.0]), np.array([np.inf, 0, 0, 0])):
        assert _apply(lib, m, 1.3, bad_q, t, fr, pt) == -22, bad_q
    for bad_s in (0.0, -1.3, float("nan"), float("inf")):
        assert _apply(lib, m, bad_s, q, t, fr, pt) == -22, bad_s
    assert _apply(lib, m, 1.3, q, np.array([0.0, np.nan, 0.0]), fr, pt) == -22
    for frames, points in (([5, m.num_frames], [1]), ([-1], [1]), ([5, 6, 5], [1]), ([5], [m.num_points]), ([5], [-1]),
                           ([5], [1, 2, 1])):
        assert _apply(lib, m, 1.3, q, t, frames, points) == -22, (frames, points)
    assert lib.sg_last_error()
    assert _arrays(m) == before
    assert _apply(lib, m, 1.3, q, t, [], []) == 0 and _arrays(m) == before      # empty lists: a no-op
    assert _apply(lib, m, 1.3, q * (1 + 1e-12), t, [5], [1]) == 0               # unit to rounding is accepted


@pytest.mark.parametrize("kind", ["sim", "rigid"])
def test_apply_similarity_takes_set_a_onto_set_b(kind):
    lib = load_library()
    m, corr, _ = ac.scene("exact", 0.0, kind)
    assert _apply(lib, m, ac.SCALES[kind], quat_from_matrix(ac.R_TRUE), ac.T_TRUE, [], corr[:, 0]) == 0
    d = np.linalg.norm(ac.euclid(m, corr[:, 0]) - ac.euclid(m, corr[:, 1]), axis=1).max()
    print("%s: A moved onto B within %.3e" % (kind, d))
    assert d <= ac.MARGIN * ac.SPREAD_EXACT["resid"]
