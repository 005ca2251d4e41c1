"""Cases and the numpy reference of keyframe retrieval, sg_matcher_db_query (include/slamgpu.h).  Test material only:
nothing here is a path of the library.

A case is a list of descriptor sets (the database, in order of addition), a query, the options, k and a skip mask.
reference() is the contract's rules 1-6 written plainly with numpy: distances by bitwise_count, best and second per
(set, query), acceptance, the one-to-one rule, scores, ranking, match rows.  Its `off` argument switches single rules
off ("ratio", "max_dist", "unique", "tie"), for the tests that show each planted case bites.

Shapes are the smallest at which the kernels can go wrong: T = 128 is the LDS tile, L = 1024 the slice length (a set
longer than L is cut into several work items), Q = 256 the queries of one workgroup."""
import functools
from types import SimpleNamespace

import numpy as np

from slamgpu.matcher import make_descriptor_sets

T = 128       # kRetrieveTile of csrc/retrieve_plan.h (held equal by test_retrieve_plan.py)
L = 1024      # kRetrieveSlice
Q = 256       # kRetrieveQ
DEFAULTS = dict(max_dist=64, ratio_percent=80, min_score=1)


def _rows(rng, n):
    return rng.integers(0, 2 ** 64, size=(n, 4), dtype=np.uint64, endpoint=False)


def flip(row, bits):
    """The descriptor `row` with the listed bit positions (0..255) flipped."""
    r = np.array(row, dtype=np.uint64).copy()
    for b in bits:
        r[b >> 6] ^= np.uint64(1) << np.uint64(b & 63)
    return r


def distances(q, t):
    """popcount(q XOR t) for every (query row, set row): (nq, n) int64."""
    q, t = np.asarray(q, np.uint64).reshape(-1, 4), np.asarray(t, np.uint64).reshape(-1, 4)
    return np.bitwise_count(q[:, None, :] ^ t[None, :, :]).sum(-1).astype(np.int64)


def _case(sets, query, k, options=None, skip=None):
    o = dict(DEFAULTS)
    o.update(options or {})
    return SimpleNamespace(sets=[np.ascontiguousarray(s, np.uint64).reshape(-1, 4) for s in sets],
                           query=np.ascontiguousarray(query, np.uint64).reshape(-1, 4), k=k, options=o,
                           skip=None if skip is None else np.asarray(skip, np.uint8))


def variant(case, **kw):
    """The case with some fields replaced (sets, query, k, options, skip)."""
    d = dict(vars(case))
    d.update(kw)
    return SimpleNamespace(**d)


# ------------------------------------------------------------------------------------------------ the reference
def reference_set(t, q, o, off=()):
    """Rules 1-4 for one set: (match, match_dist, score, candidates, losing claims)."""
    nq, n = len(q), len(t)
    match, dist = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
    if n == 0 or nq == 0:
        return match, dist, 0, 0, 0
    d = distances(q, t)
    rows = np.arange(nq)
    bd = d.min(1)
    if "tie" in off:
        bi = n - 1 - d[:, ::-1].argmin(1)          # the highest index of the minimum
    else:
        bi = d.argmin(1)                           # rule 1: the lowest
    if n >= 2:
        rest = d.copy()
        rest[rows, bi] = 1 << 30
        sd = rest.min(1)                           # the multiset's second smallest: equal to bd on a tie
    else:
        sd = np.full(nq, -1, np.int64)
    cand = np.ones(nq, bool)
    if "max_dist" not in off:
        cand &= bd <= o["max_dist"]
    if "ratio" not in off:
        cand &= (sd < 0) | (100 * bd <= o["ratio_percent"] * sd)
    winners = cand.copy()
    if "unique" not in off:
        for j in np.unique(bi[cand]):
            claimants = rows[cand & (bi == j)]
            order = sorted(claimants, key=lambda i: (bd[i], i))
            winners[order[1:]] = False             # rule 3: no fall-back
    match[winners], dist[winners] = bi[winners], bd[winners]
    return match, dist, int(winners.sum()), int(cand.sum()), int(cand.sum() - winners.sum())


def rank(score, skip, min_score, k):
    """Rule 5."""
    order = sorted((s for s in range(len(score)) if not (skip is not None and skip[s]) and score[s] >= min_score),
                   key=lambda s: (-score[s], s))
    top_set, top_score = np.full(k, -1, np.int32), np.full(k, -1, np.int32)
    for r, s in enumerate(order[:k]):
        top_set[r], top_score[r] = s, score[s]
    return top_set, top_score


def reference(case, off=()):
    """The contract on one case: score [S], top_set [k], top_score [k], match [k, nq], match_dist [k, nq]; and, for
    the tests of the cases themselves, per set the match row (cells), the candidates and the losing claims."""
    o, q, S, nq = case.options, case.query, len(case.sets), len(case.query)
    score = np.zeros(S, np.int32)
    cells, cands, losing = [], [], []
    for s, t in enumerate(case.sets):
        if case.skip is not None and case.skip[s]:
            score[s] = -1
            cells.append(None)
            cands.append(0)
            losing.append(0)
            continue
        m, d, sc, nc, nl = reference_set(t, q, o, off)
        score[s] = sc
        cells.append((m, d))
        cands.append(nc)
        losing.append(nl)
    top_set, top_score = rank(score, case.skip, o["min_score"], case.k)
    match, dist = np.full((case.k, nq), -1, np.int32), np.full((case.k, nq), -1, np.int32)
    for r, s in enumerate(top_set):
        if s >= 0:
            match[r], dist[r] = cells[s]
    return SimpleNamespace(score=score, top_set=top_set, top_score=top_score, match=match, match_dist=dist,
                           cells=cells, candidates=cands, losing=losing)


# ------------------------------------------------------------------------------------------------ the cases
SIZES_SETS = (0, 1, 2, T - 1, T, T + 1, L, L + 1, 2 * L + 77)
SIZES_QUERIES = (1, 255, 257, 600)
SIZES_PLANT = (5, L + 9, 2 * L + 60)     # one descriptor, in all three slices of the longest set, equal to query 0


@functools.lru_cache(maxsize=None)
def _sizes_database():
    rng = np.random.default_rng(21)
    sets = [_rows(rng, n) for n in SIZES_SETS]
    for j in SIZES_PLANT[1:]:
        sets[-1][j] = sets[-1][SIZES_PLANT[0]]
    return sets


def sizes(nq):
    sets = _sizes_database()
    q = _rows(np.random.default_rng(100 + nq), nq)
    q[0] = sets[-1][SIZES_PLANT[0]]
    return _case(sets, q, k=4, options=dict(max_dist=256, ratio_percent=100))


REVISIT_SET = 3


def revisit(n=400):
    A, B, truth = make_descriptor_sets(n, seed=5)
    rng = np.random.default_rng(31)
    sets = [A if s == REVISIT_SET else _rows(rng, n) for s in range(6)]
    c = _case(sets, B, k=3)
    c.truth = truth
    return c


# planted(): query rows, by name
P_FAR, P_NEAR, P_EQ_LOW, P_EQ_HIGH, P_RATIO, P_TIE_POS, P_TIE_ZERO, P_AT_MAX, P_OVER_MAX, P_LONE = range(10)


def planted():
    """Hand-made descriptors, one query each per rule.  Set 0 = d[0..7]:
      d0: P_FAR at 10 bits and P_NEAR at 4 both claim it: the nearer wins, P_FAR is unmatched;
      d1: P_EQ_LOW and P_EQ_HIGH both at 6: the lower query index wins, the other gets -1 (no fall-back);
      d2, d3 = d2 with 44 bits flipped: P_RATIO is 20 from d2 and 24 from d3: 100 * 20 > 80 * 24, refused;
      d4 = d5: P_TIE_POS at 5 from both: best == second > 0, refused; P_TIE_ZERO equal to both: 0 <= 0, matched to
          the lower index;
      d6: P_AT_MAX at exactly max_dist = 64: accepted; d7: P_OVER_MAX at 65: refused.
    Set 1 = one descriptor e, P_LONE at 3 bits: second_dist = -1 passes the ratio rule.  Sets 2 = (d0, d1) and
    3 = (d1, d0) score 2 each: ranked by index.  Set 4 = set 0 and e scores 5 and would rank first: it is skipped.
    min_score = 2 cuts set 1 (score 1) off the ranking.  Every other pair is a random 256-bit distance (about 128)."""
    rng = np.random.default_rng(11)
    d = _rows(rng, 8)
    e = _rows(rng, 1)[0]
    d[3] = flip(d[2], range(44))
    d[5] = d[4]
    q = np.zeros((10, 4), np.uint64)
    q[P_FAR] = flip(d[0], range(10))
    q[P_NEAR] = flip(d[0], range(100, 104))
    q[P_EQ_LOW] = flip(d[1], range(6))
    q[P_EQ_HIGH] = flip(d[1], range(50, 56))
    q[P_RATIO] = flip(d[2], range(20))
    q[P_TIE_POS] = flip(d[4], range(200, 205))
    q[P_TIE_ZERO] = d[4]
    q[P_AT_MAX] = flip(d[6], range(64))
    q[P_OVER_MAX] = flip(d[7], range(65))
    q[P_LONE] = flip(e, range(3))
    sets = [d, e[None, :], d[[0, 1]], d[[1, 0]], np.concatenate([d, e[None, :]])]
    return _case(sets, q, k=5, options=dict(min_score=2), skip=[0, 0, 0, 0, 1])


GROWTH_TWINS = (2, 31)


def growth():
    """40 sets of 1 to 300 descriptors (a fresh handle's buffer doubles several times on the way), the same set at
    positions 2 and 31; the query takes noisy copies of rows of every third set, and random rows."""
    rng = np.random.default_rng(41)
    sets = [_rows(rng, int(n)) for n in rng.integers(1, 301, size=40)]
    sets[GROWTH_TWINS[1]] = sets[GROWTH_TWINS[0]].copy()
    q = []
    for s in range(0, 40, 3):
        for j in range(0, len(sets[s]), 7):
            q.append(flip(sets[s][j], rng.choice(256, size=int(rng.integers(0, 12)), replace=False)))
    q = np.array(q, np.uint64)[rng.permutation(len(q))][:280]
    q = np.concatenate([q, _rows(rng, 20)])
    return _case(sets, q, k=4)


NAMES = tuple("sizes_%d" % n for n in SIZES_QUERIES) + ("revisit", "planted", "growth")


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("sizes_"):
        return sizes(int(name[6:]))
    return {"revisit": revisit, "planted": planted, "growth": growth}[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """reference(case(name)), computed once and shared: do not write into it."""
    return reference(case(name))
