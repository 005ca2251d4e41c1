"""Argument handling of sg_slam_relative_poses, its option defaults and struct sizes: needs the library but no GPU.
(Every argument error is found by the host-only planner before the device is touched.)"""
import ctypes as C

import numpy as np

from slamgpu.capi import REL_STATUS, SgMap, SgRelposeOptions, SgRelposeResult, load_library


def _options(lib):
    o = SgRelposeOptions(threshold_px=7.0, max_hypotheses=7, min_inliers=7, min_parallax=7.0, seed=7, refine=7,
                         baseline=7.0)
    lib.sg_relpose_options_default(C.byref(o))
    return o


def test_symbols_defaults_and_struct_sizes():
    lib = load_library()
    assert lib.sg_slam_relative_poses and lib.sg_relpose_options_default
    o = _options(lib)
    assert (o.threshold_px, o.max_hypotheses, o.min_inliers, o.min_parallax, o.seed, o.refine, o.baseline) == \
        (2.0, 1024, 16, 0.0, 0, 1, 0.0)
    assert C.sizeof(SgRelposeOptions) == 40 and C.sizeof(SgRelposeResult) == 224
    assert REL_STATUS == {0: "OK", 1: "DID_NOT_RUN", 2: "NO_MODEL", 3: "FEW_INLIERS", 4: "NO_CHEIRALITY",
                          5: "LOW_PARALLAX"}


def _map():
    """Two frames on one camera, no observations: held in a tuple so the arrays outlive the struct."""
    k = np.array([0, 0, 0, 416.0, -416.0, 320.0, 240.0])
    q, t = np.tile([0.0, 0, 0, 1], 2), np.zeros(6)
    cam, prev = np.zeros(2, dtype=np.int32), np.full(2, -1, dtype=np.int32)
    m = SgMap()
    m.num_cameras, m.num_frames = 1, 2
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    m.k, m.q, m.t = k.ctypes.data_as(dp), q.ctypes.data_as(dp), t.ctypes.data_as(dp)
    m.frame_camera, m.frame_prev = cam.ctypes.data_as(ip), prev.ctypes.data_as(ip)
    return m, (k, q, t, cam, prev)


def test_argument_errors_return_before_the_device_is_touched():
    lib = load_library()
    f = lib.sg_slam_relative_poses
    m, keep = _map()
    buf = C.create_string_buffer(64)
    dummy = C.cast(buf, C.c_void_p)   # an opaque non-null handle: it must never be touched
    before = bytes(buf.raw)
    pairs = (C.c_int32 * 2)(0, 1)
    solved = (C.c_int32 * 1)(7)

    def call(handle, mp, pr, n, o):
        return f(handle, mp, pr, n, o, solved, None, None, None, None, 0)

    o = _options(lib)
    assert call(None, C.byref(m), pairs, 1, C.byref(o)) == -22
    assert call(dummy, None, pairs, 1, C.byref(o)) == -22
    assert call(dummy, C.byref(m), pairs, 1, None) == -22
    assert call(dummy, C.byref(m), None, 0, None) == -22          # null options, even with n == 0
    assert call(dummy, C.byref(m), pairs, -1, C.byref(o)) == -22
    for field, bad in (("threshold_px", 0.0), ("threshold_px", -1.0), ("threshold_px", float("nan")),
                       ("max_hypotheses", 0), ("max_hypotheses", -256), ("baseline", -1.0)):
        b = _options(lib)
        setattr(b, field, bad)
        assert call(dummy, C.byref(m), pairs, 1, C.byref(b)) == -22, (field, bad)
        assert call(dummy, C.byref(m), None, 0, C.byref(b)) == -22, (field, bad)
    for a, b in ((0, 2), (-1, 1), (1, 1)):
        assert call(dummy, C.byref(m), (C.c_int32 * 2)(a, b), 1, C.byref(o)) == -22, (a, b)
    assert call(dummy, C.byref(m), (C.c_int32 * 4)(0, 1, 0, 1), 2, C.byref(o)) == -22    # the same b twice
    assert lib.sg_last_error()
    assert call(dummy, C.byref(m), None, 0, C.byref(o)) == 0      # n == 0: a no-op
    assert solved[0] == 7 and bytes(buf.raw) == before
    del keep
