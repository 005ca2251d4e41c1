"""Argument handling of sg_slam_triangulate_points and its option defaults: needs the library but no GPU."""
import ctypes as C

import numpy as np

from slamgpu.capi import SgMap, SgSolverSummary, SgTriangulateOptions, SgTriangulateResult, load_library


def _options(lib):
    o = SgTriangulateOptions(min_parallax=7.0, max_error_px=7.0, refine=7, range=7.0)
    lib.sg_triangulate_options_default(C.byref(o))
    return o


def test_option_defaults():
    o = _options(load_library())
    assert (o.min_parallax, o.max_error_px, o.refine, o.range) == (0.0, 0.0, 0, 2.0)
    assert C.sizeof(SgTriangulateOptions) == 32 and C.sizeof(SgTriangulateResult) == 64


def test_null_handle_map_or_options_returns_einval():
    lib = load_library()
    o = _options(lib)
    points = (C.c_int32 * 1)(0)
    solved = (C.c_int32 * 1)(7)
    m = SgMap()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)   # a non-null handle: the arguments are checked first
    f = lib.sg_slam_triangulate_points
    assert f(None, C.byref(m), points, 1, C.byref(o), solved, None, None) == -22
    assert f(dummy, None, points, 1, C.byref(o), solved, None, None) == -22
    assert f(dummy, C.byref(m), points, 1, None, solved, None, None) == -22
    assert f(None, None, None, 0, None, None, None, None) == -22
    assert f(dummy, C.byref(m), None, 0, None, None, None, None) == -22   # null options, even with n == 0
    assert solved[0] == 7
    assert lib.sg_last_error()


def test_zero_points_is_a_no_op_without_a_device():
    lib = load_library()
    o = _options(lib)
    # n == 0 returns before the handle or the device is touched, so an opaque non-null handle stands in for an
    # sg_slam (sg_slam_create itself needs a device)
    buf = C.create_string_buffer(64)
    dummy = C.cast(buf, C.c_void_p)
    m = SgMap()
    sums = (SgSolverSummary * 1)()
    res = (SgTriangulateResult * 1)()
    res[0].status = 7
    before = bytes(buf.raw)
    f = lib.sg_slam_triangulate_points
    assert f(dummy, C.byref(m), None, 0, C.byref(o), None, None, None) == 0
    points = np.zeros(1, dtype=np.int32)
    solved = np.full(1, 7, dtype=np.int32)
    assert f(dummy, C.byref(m), points.ctypes.data_as(C.POINTER(C.c_int32)), 0, C.byref(o),
             solved.ctypes.data_as(C.POINTER(C.c_int32)), res, sums) == 0
    assert solved[0] == 7 and res[0].status == 7 and bytes(buf.raw) == before


def test_negative_count_returns_einval():
    lib = load_library()
    o = _options(lib)
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    m = SgMap()
    assert lib.sg_slam_triangulate_points(dummy, C.byref(m), None, -1, C.byref(o), None, None, None) == -22
