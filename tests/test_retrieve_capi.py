"""The keyframe database's entry points (sg_matcher_db_*), its option defaults and struct layout: needs the library but
no GPU."""
import ctypes as C

import numpy as np

from slamgpu.capi import SgRetrieveOptions, load_library

IP, UP = C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
NAMES = ("sg_matcher_db_add", "sg_matcher_db_clear", "sg_matcher_db_count", "sg_retrieve_options_default",
         "sg_matcher_db_query", "sg_matcher_db_query_ms")


def test_symbols_defaults_and_struct_layout():
    lib = load_library()
    for n in NAMES:
        assert getattr(lib, n), n
    o = SgRetrieveOptions(max_dist=7, ratio_percent=7, min_score=7)
    lib.sg_retrieve_options_default(C.byref(o))
    assert (o.max_dist, o.ratio_percent, o.min_score) == (64, 80, 1)
    lib.sg_retrieve_options_default(None)                                # a null pointer is ignored
    # the C layout: three 32-bit fields
    assert C.sizeof(SgRetrieveOptions) == 12
    assert [getattr(SgRetrieveOptions, n).offset for n, _ in SgRetrieveOptions._fields_] == [0, 4, 8]


def test_a_null_handle_is_einval_from_every_entry_point():
    lib = load_library()
    desc = np.arange(8, dtype=np.uint64)
    sid, ns, nd, ms = C.c_int32(7), C.c_int32(7), C.c_int64(7), C.c_double(7.0)
    o = SgRetrieveOptions()
    lib.sg_retrieve_options_default(C.byref(o))
    outs = [np.full(2, 7, dtype=np.int32) for _ in range(5)]
    assert lib.sg_matcher_db_add(None, desc.ctypes.data_as(UP), 2, C.byref(sid)) == -22
    assert lib.sg_matcher_db_clear(None) == -22
    assert lib.sg_matcher_db_count(None, C.byref(ns), C.byref(nd)) == -22
    assert lib.sg_matcher_db_query(None, desc.ctypes.data_as(UP), 2, C.byref(o), None, outs[0].ctypes.data_as(IP), 1,
                                   outs[1].ctypes.data_as(IP), outs[2].ctypes.data_as(IP), outs[3].ctypes.data_as(IP),
                                   outs[4].ctypes.data_as(IP)) == -22
    assert lib.sg_matcher_db_query_ms(None, C.byref(ms)) == -22
    assert lib.sg_last_error()
    # nothing written
    assert (sid.value, ns.value, nd.value, ms.value) == (7, 7, 7, 7.0) and all((x == 7).all() for x in outs)
