"""Argument handling of sg_slam_match_epipolar, its option defaults, struct layouts and the agreement of the header, the
ctypes table and the Python wrapper: needs the library but no GPU.  (Every argument error is found by the host-only
planner before the device is touched.)  The planner's CPU executor, reached through the library's diagnostic entry
point, must also equal the numpy reference on every case."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import epipolar_cases as ec
from slamgpu import ba
from slamgpu.capi import SYMBOLS, SgEpipolarOptions, SgEpipolarResult, SgMap, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IP, DP, UP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
MAP_ARRAYS = ("k", "q", "t", "X", "point_flags", "point_uncertainty", "obs_pt", "obs_frame", "obs_point",
              "obs_disabled", "obs_error", "frame_camera", "frame_prev")


def _options(lib):
    o = SgEpipolarOptions(tol_px=7.0, min_parallax=7.0, max_dist=7, ratio_percent=7)
    lib.sg_epipolar_options_default(C.byref(o))
    return o


def test_symbols_defaults_and_struct_layouts():
    lib = load_library()
    assert lib.sg_slam_match_epipolar and lib.sg_epipolar_options_default
    o = _options(lib)
    assert (o.tol_px, o.min_parallax, o.max_dist, o.ratio_percent) == (2.0, 0.0, 64, 80)
    # the C layouts: two doubles and two 32-bit fields | five ints
    assert C.sizeof(SgEpipolarOptions) == 24 and C.sizeof(SgEpipolarResult) == 20
    assert [getattr(SgEpipolarOptions, n).offset for n, _ in SgEpipolarOptions._fields_] == [0, 8, 16, 20]
    assert [getattr(SgEpipolarResult, n).offset for n, _ in SgEpipolarResult._fields_] == [0, 4, 8, 12, 16]


def test_header_ctypes_and_wrapper_agree():
    src = open(os.path.join(ROOT, "include", "slamgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"int sg_slam_match_epipolar\((.*?)\);", code, flags=re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    kinds = {"sg_slam*": C.c_void_p, "const sg_map*": C.POINTER(SgMap), "const int32_t*": IP, "int32_t*": IP,
             "int32_t": C.c_int32, "const double*": DP, "const uint64_t*": UP,
             "const sg_epipolar_options*": C.POINTER(SgEpipolarOptions), "sg_epipolar_result*": C.POINTER(SgEpipolarResult)}
    want = [kinds[p.rsplit(" ", 1)[0]] for p in params]
    res, args = SYMBOLS["sg_slam_match_epipolar"]
    assert res is C.c_int and args == want
    assert [p.rsplit(" ", 1)[1] for p in params] == [
        "s", "map", "pairs", "n", "a_offset", "a_xy", "a_desc", "a_level", "b_offset", "b_xy", "b_desc", "b_level",
        "options", "match", "best_kp", "best_dist", "second_dist", "num_candidates", "results"]
    for struct, name in ((SgEpipolarOptions, "sg_epipolar_options"), (SgEpipolarResult, "sg_epipolar_result")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), code, flags=re.S).group(1)
        fields = [f.strip() for stmt in body.split(";") if stmt.strip()
                  for f in stmt.strip().split(" ", 1)[1].split(",")]
        assert fields == [n for n, _ in struct._fields_], name
    assert SYMBOLS["sg_epipolar_options_default"] == (None, [C.POINTER(SgEpipolarOptions)])
    # the wrapper's defaults are the library's
    sig = inspect.signature(ba.Slam.MatchEpipolar).parameters
    o = _options(load_library())
    assert [sig[n].default for n in ("tol_px", "min_parallax", "max_dist", "ratio_percent")] == \
        [o.tol_px, o.min_parallax, o.max_dist, o.ratio_percent]
    assert list(sig)[:5] == ["self", "m", "pairs", "keypoints_a", "keypoints_b"]
    assert callable(ba.Slam.epipolar_match_results)


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_cpu_executor_equals_the_reference(name):
    c, want = ec.case(name), ec.expected(name)
    got = ba.match_epipolar_cpu(c.m, c.pairs, ec.call_keypoints(c, "a"), ec.call_keypoints(c, "b"), **c.options)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert all(g[k] == w[k] for k in ec.COUNTS)
        assert all(np.array_equal(g[k], w[k]) and g[k].dtype == np.int32 for k in ec.ARRAYS)


def _flat(kps):
    off = np.zeros(len(kps) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(k[0]) for k in kps])
    return (off, np.concatenate([k[0] for k in kps]).reshape(-1), np.concatenate([k[1] for k in kps]).reshape(-1),
            np.concatenate([k[2] for k in kps]).astype(np.int32))


def test_argument_errors_return_before_the_device_is_touched():
    lib = load_library()
    f = lib.sg_slam_match_epipolar
    c = ec.case("planted")
    m = c.m.copy()
    before = {n: getattr(m, n).tobytes() for n in MAP_ARRAYS}
    ms = m.struct()
    buf = C.create_string_buffer(64)
    dummy = C.cast(buf, C.c_void_p)   # an opaque non-null handle: it must never be touched
    raw = bytes(buf.raw)
    pairs = np.array(c.pairs, dtype=np.int32).reshape(-1)
    n = len(c.pairs)
    ao, axy, ad, al = _flat(c.keypoints_a)
    bo, bxy, bd, bl = _flat(c.keypoints_b)
    KA = int(ao[-1])
    outs = [np.full(KA, 7, dtype=np.int32) for _ in range(5)]
    res = (SgEpipolarResult * n)()
    res[0].num_b = 77
    good = dict(handle=dummy, mp=C.byref(ms), pairs=pairs, n=n, ao=ao, axy=axy, ad=ad, al=al, bo=bo, bxy=bxy, bd=bd,
                bl=bl, match=outs[0])

    def call(opt, **kw):
        a = dict(good)
        a.update(kw)
        p = lambda v, t: None if v is None else v.ctypes.data_as(t)   # noqa: E731
        return f(a["handle"], a["mp"], p(a["pairs"], IP), a["n"], p(a["ao"], IP), p(a["axy"], DP), p(a["ad"], UP),
                 p(a["al"], IP), p(a["bo"], IP), p(a["bxy"], DP), p(a["bd"], UP), p(a["bl"], IP), opt,
                 p(a["match"], IP), *[p(x, IP) for x in outs[1:]], res)

    o = C.byref(_options(lib))
    for kw in (dict(handle=None), dict(mp=None), dict(match=None), dict(n=-1), dict(pairs=None), dict(ao=None),
               dict(bo=None), dict(axy=None), dict(ad=None), dict(bxy=None), dict(bd=None), dict(al=None), dict(bl=None)):
        assert call(o, **kw) == -22, kw
    assert call(None) == -22
    assert call(None, n=0) == -22                                      # null options, even with n == 0
    assert call(o, match=None, n=0) == -22
    for arr in ("ao", "bo"):
        bad = good[arr].copy()
        bad[0] = 1
        assert call(o, **{arr: bad}) == -22
        bad = good[arr].copy()
        bad[1] = bad[2] + 1
        assert call(o, **{arr: bad}) == -22
        big = np.array([0, 2 ** 20 + 1], dtype=np.int32)
        assert call(o, n=1, **{arr: big, ("bo" if arr == "ao" else "ao"): np.zeros(2, dtype=np.int32)}) == -22
    for arr in ("al", "bl"):
        for v in (-1, 8):
            bad = good[arr].copy()
            bad[3] = v
            assert call(o, **{arr: bad}) == -22, (arr, v)
    for slot in (0, 1):
        for v in (-1, m.num_frames, 2 ** 31 - 1):
            b = pairs.copy()
            b[2 + slot] = v
            assert call(o, pairs=b) == -22, v
    b = pairs.copy()
    b[5] = b[4]
    assert call(o, pairs=b) == -22                                     # a == b
    for field, v in (("tol_px", 0.0), ("tol_px", -2.0), ("tol_px", float("nan")), ("tol_px", float("inf")),
                     ("min_parallax", -0.1), ("min_parallax", float("nan")), ("min_parallax", float("inf")),
                     ("max_dist", -1), ("max_dist", 257), ("ratio_percent", 0), ("ratio_percent", 101)):
        b = _options(lib)
        setattr(b, field, v)
        assert call(C.byref(b)) == -22, (field, v)
        assert call(C.byref(b), n=0) == -22, (field, v)
    # partial results above 128 MiB: 2^20 a keypoints against 9 slices of b keypoints (the arrays are then not read)
    assert call(o, n=1, ao=np.array([0, 2 ** 20], dtype=np.int32), bo=np.array([0, 8 * ec.SLICE + 1], dtype=np.int32),
                al=None, bl=None) == -22
    # maps that cannot be read
    for name in ("q", "t", "k", "frame_camera"):
        broken = m.struct()
        setattr(broken, name, None)
        assert call(o, mp=C.byref(broken)) == -22, name
    m2 = m.copy()
    m2.frame_camera[c.pairs[0][1]] = 2
    ms2 = m2.struct()
    assert call(o, mp=C.byref(ms2)) == -22                             # a camera index out of range
    assert lib.sg_last_error()
    assert call(o, n=0) == 0                                           # n == 0: a no-op, without a device
    assert call(o, n=0, pairs=None, ao=None, axy=None, ad=None, al=None, bo=None, bxy=None, bd=None, bl=None) == 0
    # a failing call writes nothing: the map, the handle and every output are as they were
    assert all((x == 7).all() for x in outs) and res[0].num_b == 77 and bytes(buf.raw) == raw
    assert {n_: getattr(m, n_).tobytes() for n_ in MAP_ARRAYS} == before


def test_calls_without_a_live_pair_need_no_device():
    """Every pair empty or degenerate: nothing is launched, so the answer comes without the handle being touched."""
    lib = load_library()
    f = lib.sg_slam_match_epipolar
    c = ec.case("planted")
    ms = c.m.struct()
    buf = C.create_string_buffer(64)
    dummy, raw = C.cast(buf, C.c_void_p), bytes(buf.raw)
    o = _options(lib)
    a, b = c.keypoints_a[0], c.keypoints_b[0]
    na, nb = len(a[0]), len(b[0])
    # pair 0 has no b keypoints, pair 1 no a keypoints, pair 2 is the zero-baseline pair with both
    pairs = np.array([ec.PLANT_PAIR, ec.PLANT_PAIR, ec.ZERO_PAIR], dtype=np.int32).reshape(-1)
    ao, bo = np.array([0, na, na, 2 * na], dtype=np.int32), np.array([0, 0, nb, 2 * nb], dtype=np.int32)
    axy, ad = np.concatenate([a[0], a[0]]).reshape(-1), np.concatenate([a[1], a[1]]).reshape(-1)
    bxy, bd = np.concatenate([b[0], b[0]]).reshape(-1), np.concatenate([b[1], b[1]]).reshape(-1)
    outs = [np.full(2 * na, 7, dtype=np.int32) for _ in range(5)]
    res = (SgEpipolarResult * 3)()
    assert f(dummy, C.byref(ms), pairs.ctypes.data_as(IP), 3, ao.ctypes.data_as(IP), axy.ctypes.data_as(DP),
             ad.ctypes.data_as(UP), None, bo.ctypes.data_as(IP), bxy.ctypes.data_as(DP), bd.ctypes.data_as(UP), None,
             C.byref(o), *[x.ctypes.data_as(IP) for x in outs], res) == 0
    assert all((x == -1).all() for x in outs[:4]) and (outs[4] == 0).all()
    assert [tuple(getattr(r, k) for k in ec.COUNTS) for r in res] == [(na, 0, 0, 0, 0), (0, nb, 0, 0, 0), (na, nb, 0, 0, 1)]
    # the optional outputs may be null
    match = np.full(2 * na, 7, dtype=np.int32)
    assert f(dummy, C.byref(ms), pairs.ctypes.data_as(IP), 3, ao.ctypes.data_as(IP), axy.ctypes.data_as(DP),
             ad.ctypes.data_as(UP), None, bo.ctypes.data_as(IP), bxy.ctypes.data_as(DP), bd.ctypes.data_as(UP), None,
             C.byref(o), match.ctypes.data_as(IP), None, None, None, None, None) == 0
    assert (match == -1).all() and bytes(buf.raw) == raw
