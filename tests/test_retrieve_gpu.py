"""Keyframe retrieval on the device (sg_matcher_db_*) against the numpy reference of tests/retrieve_cases.py: every
output equal in every element on every case, the same bytes on a second query, data that survives the buffer's
reallocations, twins with identical answers, clear and re-add, skip, the SG_EINVAL cases that depend on the database's
state, the empty shapes, and independence from sg_hamming_match on the same handle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import oracle  # noqa: E402
import retrieve_cases as rc  # noqa: E402
from slamgpu.capi import SgRetrieveOptions  # noqa: E402
from slamgpu.matcher import HammingMatcher  # noqa: E402

pytestmark = pytest.mark.gpu
IP, UP, BP = C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
FIELDS = ("score", "top_set", "top_score", "match", "match_dist")


def _loaded(case):
    m = HammingMatcher()
    ids = [m.add_keyframe(s) for s in case.sets]
    assert ids == list(range(len(case.sets)))
    assert m.keyframe_count() == (len(case.sets), sum(len(s) for s in case.sets))
    return m


def _query(m, case, **kw):
    a = dict(k=case.k, skip=case.skip, **case.options)
    a.update(kw)
    return m.query_keyframes(case.query, **a)


def _assert_equal(got, want, what=""):
    for name, g in zip(FIELDS, got):
        np.testing.assert_array_equal(g, getattr(want, name), err_msg="%s %s" % (what, name))


def _rows_by_set(m, case, skip=None):
    """Every set's match row: all sets rank with k = S and min_score = 0."""
    S = len(case.sets)
    score, top_set, _, match, dist = m.query_keyframes(case.query, k=S, skip=skip, **dict(case.options, min_score=0))
    rows = {int(s): (match[r].copy(), dist[r].copy()) for r, s in enumerate(top_set) if s >= 0}
    return score, rows


def _raw_query(m, q, nq, S, k, options=(64, 80, 1), skip=None, want_rows=True, fill=7):
    """sg_matcher_db_query itself, on outputs pre-filled with `fill`: (code, score, top_set, top_score, match, dist)."""
    o = SgRetrieveOptions(*options)
    outs = [np.full(max(S, 1), fill, np.int32), np.full(max(k, 1), fill, np.int32), np.full(max(k, 1), fill, np.int32),
            np.full(max(k * min(nq, 4096), 1), fill, np.int32), np.full(max(k * min(nq, 4096), 1), fill, np.int32)]
    p = [x.ctypes.data_as(IP) for x in outs]
    if not want_rows:
        p[3] = p[4] = None
    rc_ = m.lib.sg_matcher_db_query(m.h, None if q is None else q.ctypes.data_as(UP), nq, C.byref(o),
                                    None if skip is None else skip.ctypes.data_as(BP), *p[:1], k, *p[1:])
    return (rc_, *outs)


@pytest.mark.parametrize("name", rc.NAMES)
def test_every_output_equals_the_reference(gpu_lib, name):
    case, want = rc.case(name), rc.expected(name)
    m = _loaded(case)
    first = _query(m, case)
    ms = m.query_keyframes_ms()
    second = _query(m, case)
    print(name, "scores", first[0].tolist(), "top", first[1].tolist(), "launches %.3f ms" % ms)
    _assert_equal(first, want, name)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()                               # two consecutive queries: identical bytes
    assert ms > 0.0
    m.close()


def test_growth_survives_reallocation_twins_clear_and_skip(gpu_lib):
    case, want = rc.case("growth"), rc.expected("growth")
    m = HammingMatcher()
    assert m.keyframe_count() == (0, 0)
    for s, t in enumerate(case.sets):
        assert m.add_keyframe(t) == s
        if (s + 1) % 5 == 0:                                            # a query after every fifth addition
            part = rc.variant(case, sets=case.sets[:s + 1])
            _assert_equal(_query(m, part), rc.reference(part), "after %d sets" % (s + 1))
    full = _query(m, case)
    _assert_equal(full, want, "all sets")
    # the twins: identical scores and rows, wherever they stand
    score, rows = _rows_by_set(m, case)
    a, b = rc.GROWTH_TWINS
    assert score[a] == score[b] == want.score[a]
    assert (rows[a][0] == rows[b][0]).all() and (rows[a][1] == rows[b][1]).all()
    for s in range(len(case.sets)):
        np.testing.assert_array_equal(rows[s][0], want.cells[s][0], err_msg="set %d" % s)
        np.testing.assert_array_equal(rows[s][1], want.cells[s][1], err_msg="set %d" % s)
    # skip changes the skipped sets' entries and the ranking, nothing else
    skip = np.zeros(len(case.sets), np.uint8)
    skip[[int(full[1][0]), 2, 7, 39]] = 1                               # the best set among them
    skipped = rc.variant(case, skip=skip)
    got = _query(m, skipped)
    _assert_equal(got, rc.reference(skipped), "skip")
    assert (got[0][skip == 1] == -1).all() and (got[0][skip == 0] == full[0][skip == 0]).all()
    assert got[1][0] != full[1][0]
    score_s, rows_s = _rows_by_set(m, case, skip=skip)
    assert sorted(rows_s) == [s for s in range(len(case.sets)) if not skip[s]]
    for s in rows_s:
        assert (rows_s[s][0] == rows[s][0]).all() and (rows_s[s][1] == rows[s][1]).all()
    # clear, then the same sets again: ids from 0, the same answers
    m.clear_keyframes()
    assert m.keyframe_count() == (0, 0)
    assert [m.add_keyframe(t) for t in case.sets] == list(range(len(case.sets)))
    again = _query(m, case)
    for x, y in zip(full, again):
        assert x.tobytes() == y.tobytes()
    m.close()


def test_state_dependent_argument_errors_write_nothing(gpu_lib):
    m = HammingMatcher()
    one = np.arange(4, dtype=np.uint64)
    sid = C.c_int32(7)
    # an oversize set
    big = np.zeros((65537, 4), np.uint64)
    assert m.lib.sg_matcher_db_add(m.h, big.ctypes.data_as(UP), 65537, C.byref(sid)) == -22
    assert sid.value == 7 and m.keyframe_count() == (0, 0)
    assert m.add_keyframe(big[:65536]) == 0 and m.keyframe_count() == (1, 65536)
    m.clear_keyframes()
    # S nq above 2^23: nine sets, 2^20 queries (the query is not read)
    for s in range(9):
        assert m.add_keyframe(one) == s
    q = np.zeros((2 ** 20, 4), np.uint64)
    code, *outs = _raw_query(m, q, 2 ** 20, 9, 2)
    assert code == -22 and all((x == 7).all() for x in outs)
    code, *outs = _raw_query(m, q, 2 ** 20 + 1, 1, 2)
    assert code == -22 and all((x == 7).all() for x in outs)
    code, score, *_ = _raw_query(m, q, 2 ** 20 - 2 ** 17, 9, 0, want_rows=False)   # just below: runs
    assert code == 0 and (score[:9] == 1).all()                          # every zero row claims the one descriptor
    # too many sets
    m.clear_keyframes()
    empty = np.zeros((0, 4), np.uint64)
    for s in range(4096):
        rc_ = m.lib.sg_matcher_db_add(m.h, empty.ctypes.data_as(UP), 0, None)
        assert rc_ == 0, s
    assert m.lib.sg_matcher_db_add(m.h, one.ctypes.data_as(UP), 1, C.byref(sid)) == -22
    assert sid.value == 7 and m.keyframe_count() == (4096, 0)
    assert m.lib.sg_last_error()
    m.close()


def test_empty_shapes_k_zero_and_null_rows(gpu_lib):
    case, want = rc.case("planted"), rc.expected("planted")
    S, nq = len(case.sets), len(case.query)
    opts = tuple(case.options[n] for n in ("max_dist", "ratio_percent", "min_score"))
    q = case.query
    # an empty database: before the first add, and after a clear
    m = HammingMatcher()
    code, score, top_set, top_score, match, dist = _raw_query(m, q, nq, 0, 2, opts)
    assert code == 0 and (score == 7).all() and list(top_set) == [-1, -1] and list(top_score) == [-1, -1]
    assert (match[:2 * nq] == -1).all() and (dist[:2 * nq] == -1).all()
    for t in case.sets:
        m.add_keyframe(t)
    # k == 0 with null ranks and rows: the scores alone
    o = SgRetrieveOptions(*opts)
    score = np.full(S, 7, np.int32)
    assert m.lib.sg_matcher_db_query(m.h, q.ctypes.data_as(UP), nq, C.byref(o), case.skip.ctypes.data_as(BP),
                                     score.ctypes.data_as(IP), 0, None, None, None, None) == 0
    np.testing.assert_array_equal(score, want.score)
    # match == NULL, and match_dist alone
    code, score, top_set, top_score, match, dist = _raw_query(m, q, nq, S, case.k, opts, skip=case.skip, want_rows=False)
    assert code == 0 and (match == 7).all() and (dist == 7).all()
    np.testing.assert_array_equal(top_set, want.top_set)
    np.testing.assert_array_equal(top_score, want.top_score)
    dist = np.full(case.k * nq, 7, np.int32)
    assert m.lib.sg_matcher_db_query(m.h, q.ctypes.data_as(UP), nq, C.byref(o), case.skip.ctypes.data_as(BP),
                                     score.ctypes.data_as(IP), case.k, top_set.ctypes.data_as(IP),
                                     top_score.ctypes.data_as(IP), None, dist.ctypes.data_as(IP)) == 0
    np.testing.assert_array_equal(dist.reshape(case.k, nq), want.match_dist)
    # nq == 0: nothing is launched; scores 0, -1 for the skipped set, nothing ranks
    code, score, top_set, top_score, match, dist = _raw_query(m, None, 0, S, 3, opts, skip=case.skip)
    assert code == 0 and list(score) == [0, 0, 0, 0, -1] and list(top_set) == [-1] * 3 and list(top_score) == [-1] * 3
    ms = C.c_double(7.0)
    assert m.lib.sg_matcher_db_query_ms(m.h, C.byref(ms)) == 0 and ms.value == 0.0
    # a database of empty sets only: nothing to launch either; with min_score 0 they rank by index, rows of -1
    m.clear_keyframes()
    for _ in range(3):
        m.add_keyframe(np.zeros((0, 4), np.uint64))
    score, top_set, top_score, match, dist = m.query_keyframes(q, k=2, min_score=0)
    assert list(score) == [0, 0, 0] and list(top_set) == [0, 1] and list(top_score) == [0, 0]
    assert (match == -1).all() and (dist == -1).all()
    m.clear_keyframes()
    code, score, top_set, top_score, match, dist = _raw_query(m, q, nq, 0, 1, opts)
    assert code == 0 and list(top_set) == [-1] and (match[:nq] == -1).all()
    m.close()


def test_hamming_match_between_two_queries_is_independent(gpu_lib):
    case, want = rc.case("sizes_257"), rc.expected("sizes_257")
    m = _loaded(case)
    first = _query(m, case)
    rng = np.random.default_rng(3)
    q = rng.integers(0, 2 ** 64, (300, 4), dtype=np.uint64, endpoint=False)
    t = rng.integers(0, 2 ** 64, (700, 4), dtype=np.uint64, endpoint=False)
    t[500] = t[100]
    q[7] = t[100]
    got = m.match(q, t)
    for g, w in zip(got, oracle.hamming_match(q, t, nthreads=4)):
        np.testing.assert_array_equal(g, w)
    second = _query(m, case)
    _assert_equal(first, want)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    assert m.keyframe_count() == (len(case.sets), sum(len(s) for s in case.sets))
    np.testing.assert_array_equal(m.match(q, t)[0], got[0])
    m.close()
