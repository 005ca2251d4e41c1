"""Argument handling of sg_slam_localize_frames and its option defaults: needs the library but no GPU.  (A frame index
out of range or listed twice is found by the planner behind a live handle: tests/test_localize_gpu.py.)"""
import ctypes as C

import numpy as np

from slamgpu.capi import (LOC_STATUS, SgLocalizeOptions, SgLocalizeResult, SgMap, SgSolverSummary, load_library)


def _options(lib):
    o = SgLocalizeOptions(threshold_px=7.0, max_hypotheses=7, min_inliers=7, seed=7, refine=7, range=7.0)
    lib.sg_localize_options_default(C.byref(o))
    return o


def test_option_defaults_and_struct_sizes():
    o = _options(load_library())
    assert (o.threshold_px, o.max_hypotheses, o.min_inliers, o.seed, o.refine, o.range) == (4.0, 1024, 8, 0, 1, 2.0)
    assert C.sizeof(SgLocalizeOptions) == 32 and C.sizeof(SgLocalizeResult) == 120
    assert LOC_STATUS == {0: "OK", 1: "DID_NOT_RUN", 2: "NO_MODEL", 3: "FEW_INLIERS"}


def test_null_handle_map_or_options_returns_einval():
    lib = load_library()
    o = _options(lib)
    frames = (C.c_int32 * 1)(0)
    solved = (C.c_int32 * 1)(7)
    m = SgMap()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)   # a non-null handle: the arguments are checked first
    f = lib.sg_slam_localize_frames
    assert f(None, C.byref(m), frames, 1, C.byref(o), solved, None, None, None) == -22
    assert f(dummy, None, frames, 1, C.byref(o), solved, None, None, None) == -22
    assert f(dummy, C.byref(m), frames, 1, None, solved, None, None, None) == -22
    assert f(None, None, None, 0, None, None, None, None, None) == -22
    assert f(dummy, C.byref(m), None, 0, None, None, None, None, None) == -22   # null options, even with n == 0
    assert solved[0] == 7
    assert lib.sg_last_error()


def test_bad_options_and_negative_count_return_einval():
    lib = load_library()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)
    m = SgMap()
    frames = (C.c_int32 * 1)(0)
    solved = (C.c_int32 * 1)(7)
    f = lib.sg_slam_localize_frames
    assert f(dummy, C.byref(m), None, -1, C.byref(_options(lib)), None, None, None, None) == -22
    for field, bad in (("threshold_px", 0.0), ("threshold_px", -1.0), ("threshold_px", float("nan")),
                       ("max_hypotheses", 0), ("max_hypotheses", -256)):
        o = _options(lib)
        setattr(o, field, bad)
        # found before the handle is touched: the opaque handle survives, with n == 1 and with n == 0
        assert f(dummy, C.byref(m), frames, 1, C.byref(o), solved, None, None, None) == -22, (field, bad)
        assert f(dummy, C.byref(m), None, 0, C.byref(o), None, None, None, None) == -22, (field, bad)
    assert solved[0] == 7


def test_zero_frames_is_a_no_op_without_a_device():
    lib = load_library()
    o = _options(lib)
    # n == 0 returns before the handle or the device is touched, so an opaque non-null handle stands in for an
    # sg_slam (sg_slam_create itself needs a device)
    buf = C.create_string_buffer(64)
    dummy = C.cast(buf, C.c_void_p)
    m = SgMap()
    sums = (SgSolverSummary * 1)()
    res = (SgLocalizeResult * 1)()
    res[0].status = 7
    before = bytes(buf.raw)
    f = lib.sg_slam_localize_frames
    assert f(dummy, C.byref(m), None, 0, C.byref(o), None, None, None, None) == 0
    frames = np.zeros(1, dtype=np.int32)
    solved = np.full(1, 7, dtype=np.int32)
    inl = np.full(4, 7, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    assert f(dummy, C.byref(m), frames.ctypes.data_as(ip), 0, C.byref(o), solved.ctypes.data_as(ip), res,
             inl.ctypes.data_as(ip), sums) == 0
    assert solved[0] == 7 and res[0].status == 7 and (inl == 7).all() and bytes(buf.raw) == before
