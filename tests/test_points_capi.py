"""Argument handling of sg_slam_solve_points that needs the library but no GPU."""
import ctypes as C

import numpy as np

from slamgpu.capi import SgMap, SgSolverSummary, load_library


def test_null_handle_or_map_returns_einval():
    lib = load_library()
    points = (C.c_int32 * 1)(0)
    solved = (C.c_int32 * 1)(7)
    m = SgMap()
    assert lib.sg_slam_solve_points(None, C.byref(m), points, 1, 2.0, solved, None) == -22
    dummy = C.create_string_buffer(64)   # a non-null handle: the map is checked before the handle is used
    assert lib.sg_slam_solve_points(C.cast(dummy, C.c_void_p), None, points, 1, 2.0, solved, None) == -22
    assert lib.sg_slam_solve_points(None, None, None, 0, 2.0, None, None) == -22
    assert solved[0] == 7
    assert lib.sg_last_error()


def test_zero_points_is_a_no_op_without_a_device():
    lib = load_library()
    # n == 0 returns before the handle or the device is touched, so an opaque non-null handle stands in for an
    # sg_slam (sg_slam_create itself needs a device)
    dummy = C.create_string_buffer(64)
    m = SgMap()
    sums = (SgSolverSummary * 1)()
    before = bytes(dummy.raw)
    assert lib.sg_slam_solve_points(C.cast(dummy, C.c_void_p), C.byref(m), None, 0, 2.0, None, None) == 0
    points = np.zeros(1, dtype=np.int32)
    solved = np.full(1, 7, dtype=np.int32)
    assert lib.sg_slam_solve_points(C.cast(dummy, C.c_void_p), C.byref(m),
                                    points.ctypes.data_as(C.POINTER(C.c_int32)), 0, 2.0,
                                    solved.ctypes.data_as(C.POINTER(C.c_int32)), sums) == 0
    assert solved[0] == 7 and bytes(dummy.raw) == before


def test_negative_count_returns_einval():
    lib = load_library()
    dummy = C.create_string_buffer(64)
    m = SgMap()
    assert lib.sg_slam_solve_points(C.cast(dummy, C.c_void_p), C.byref(m), None, -1, 2.0, None, None) == -22
