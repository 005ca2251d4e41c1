"""The retrieval cases and their numpy reference (tests/retrieve_cases.py), checked on the CPU: every planted rule
changes the reference's answer when it is switched off, the generated cases reach every path of the kernels (partial
last tile, several slices, two query groups, losing claims), and the revisit case meets the retrieval condition: the
revisited keyframe ranks first with every kept row matched to its true row, and the random keyframes score zero.  No
GPU, no library."""
import numpy as np

import retrieve_cases as rc


def test_planted_answers_are_the_hand_made_ones():
    c, r = rc.case("planted"), rc.expected("planted")
    assert list(r.score) == [4, 1, 2, 2, -1]
    assert list(r.top_set) == [0, 2, 3, -1, -1] and list(r.top_score) == [4, 2, 2, -1, -1]
    m, d = r.match[0], r.match_dist[0]
    assert (m[rc.P_FAR], m[rc.P_NEAR], d[rc.P_NEAR]) == (-1, 0, 4)                       # the nearer claimant wins
    assert (m[rc.P_EQ_LOW], d[rc.P_EQ_LOW], m[rc.P_EQ_HIGH], d[rc.P_EQ_HIGH]) == (1, 6, -1, -1)   # no fall-back
    assert m[rc.P_RATIO] == -1 and m[rc.P_TIE_POS] == -1
    assert (m[rc.P_TIE_ZERO], d[rc.P_TIE_ZERO]) == (4, 0)                                # the lower of d4 = d5
    assert (m[rc.P_AT_MAX], d[rc.P_AT_MAX]) == (6, c.options["max_dist"]) and m[rc.P_OVER_MAX] == -1
    assert m[rc.P_LONE] == -1                                                            # e is not in set 0
    lone = r.cells[1]
    assert (lone[0][rc.P_LONE], lone[1][rc.P_LONE]) == (0, 3) and (lone[0] >= 0).sum() == 1
    assert (r.match[3:] == -1).all() and (r.match_dist[3:] == -1).all()                   # unfilled ranks
    # the distances the docstring of planted() states
    dd = rc.distances(c.query, c.sets[0])
    assert (dd[rc.P_RATIO, 2], dd[rc.P_RATIO, 3]) == (20, 24) and 100 * 20 > 80 * 24
    assert (dd[rc.P_TIE_POS, 4], dd[rc.P_TIE_POS, 5]) == (5, 5)
    assert (dd[rc.P_AT_MAX, 6], dd[rc.P_OVER_MAX, 7]) == (64, 65)
    # nothing else comes near a decision: every unplanted pair is a random distance
    planted_pairs = {(rc.P_FAR, 0), (rc.P_NEAR, 0), (rc.P_EQ_LOW, 1), (rc.P_EQ_HIGH, 1), (rc.P_RATIO, 2),
                     (rc.P_RATIO, 3), (rc.P_TIE_POS, 4), (rc.P_TIE_POS, 5), (rc.P_TIE_ZERO, 4), (rc.P_TIE_ZERO, 5),
                     (rc.P_AT_MAX, 6), (rc.P_OVER_MAX, 7)}
    others = [dd[i, j] for i in range(dd.shape[0]) for j in range(dd.shape[1]) if (i, j) not in planted_pairs]
    assert min(others) > 85


def test_each_rule_changes_the_planted_answer_when_switched_off():
    c, r = rc.case("planted"), rc.expected("planted")
    cell = r.cells[0][0]
    off = {name: rc.reference(c, off=(name,)).cells[0][0] for name in ("ratio", "max_dist", "unique", "tie")}
    assert off["ratio"][rc.P_RATIO] == 2 and cell[rc.P_RATIO] == -1
    assert off["max_dist"][rc.P_OVER_MAX] == 7 and cell[rc.P_OVER_MAX] == -1
    assert off["unique"][rc.P_FAR] == 0 and off["unique"][rc.P_EQ_HIGH] == 1
    assert off["tie"][rc.P_TIE_ZERO] == 5 and cell[rc.P_TIE_ZERO] == 4
    for name, v in off.items():
        assert (v != cell).any(), name
    # min_score, skip and the index order of equal scores decide the ranking
    assert list(rc.reference(rc.variant(c, options=dict(c.options, min_score=1))).top_set) == [0, 2, 3, 1, -1]
    unskipped = rc.reference(rc.variant(c, skip=None))
    assert list(unskipped.top_set[:2]) == [4, 0] and unskipped.score[4] == 5
    swapped = rc.reference(rc.variant(c, sets=[c.sets[i] for i in (0, 1, 3, 2, 4)]))
    assert list(swapped.top_set[:3]) == [0, 2, 3]                        # by index, whichever set stands there


def test_sizes_reach_every_path():
    assert rc.SIZES_SETS == (0, 1, 2, rc.T - 1, rc.T, rc.T + 1, rc.L, rc.L + 1, 2 * rc.L + 77)
    assert rc.L % rc.T == 0 and (2 * rc.L + 77) % rc.T != 0             # whole tiles, and a partial last tile
    assert -(-(2 * rc.L + 77) // rc.L) == 3 and -(-(rc.L + 1) // rc.L) == 2 and -(-rc.L // rc.L) == 1   # slices
    assert [n for n in rc.SIZES_QUERIES if n > rc.Q] == [257, 600] and 255 in rc.SIZES_QUERIES   # query groups
    assert sorted(j // rc.L for j in rc.SIZES_PLANT) == [0, 1, 2]       # the duplicate stands in all three slices
    for nq in rc.SIZES_QUERIES:
        c, r = rc.case("sizes_%d" % nq), rc.expected("sizes_%d" % nq)
        assert len(c.query) == nq and [len(s) for s in c.sets] == list(rc.SIZES_SETS)
        # every query is a candidate of every non-empty set
        assert r.candidates == [nq if n else 0 for n in rc.SIZES_SETS]
        assert r.score[0] == 0 and (r.score[1:] >= 1).all() and (r.score <= np.minimum(nq, rc.SIZES_SETS)).all()
        # the tie across slices: the lowest index wins and second == best == 0
        big = r.cells[-1]
        assert (big[0][0], big[1][0]) == (rc.SIZES_PLANT[0], 0)
        if nq >= 255:
            # hundreds of losing claims on the small sets, from both query groups where there are two
            for s in range(1, 6):
                assert r.losing[s] >= nq - rc.SIZES_SETS[s] and r.losing[s] >= 100
        if nq > rc.Q:
            best = rc.distances(c.query, c.sets[3]).argmin(1)           # the set of T - 1
            assert set(best[:rc.Q]) & set(best[rc.Q:])                  # two query groups claim the same descriptors
        if nq == 600:
            small = r.cells[3][0]
            assert (small[:rc.Q] >= 0).any() and (small[rc.Q:] >= 0).any()   # and each group wins some


def test_revisit_meets_the_retrieval_condition():
    c, r = rc.case("revisit"), rc.expected("revisit")
    kept = c.truth >= 0
    assert [len(s) for s in c.sets] == [400] * 6 and c.options == rc.DEFAULTS
    assert r.top_set[0] == rc.REVISIT_SET and list(r.top_set[1:]) == [-1, -1]
    m = r.match[0]
    wrong = int(((m >= 0) & (m != c.truth)).sum())
    print("kept %d, score %d, wrong %d, scores %s" % (kept.sum(), r.score[rc.REVISIT_SET], wrong, list(r.score)))
    assert wrong == 0 and (m[kept] == c.truth[kept]).all()              # every kept row, each to its true row
    assert r.score[rc.REVISIT_SET] == kept.sum() == 288
    assert all(r.score[s] == 0 for s in range(6) if s != rc.REVISIT_SET)
    nearest = min(rc.distances(c.query, c.sets[s]).min() for s in range(6) if s != rc.REVISIT_SET)
    assert nearest > c.options["max_dist"] + 16


def test_growth_has_twins_and_live_scores():
    c, r = rc.case("growth"), rc.expected("growth")
    a, b = rc.GROWTH_TWINS
    assert len(c.sets) == 40 and all(1 <= len(s) <= 300 for s in c.sets)
    assert (c.sets[a] == c.sets[b]).all() and r.score[a] == r.score[b]
    assert (r.cells[a][0] == r.cells[b][0]).all() and (r.cells[a][1] == r.cells[b][1]).all()
    assert (r.score[::3] >= 5).all() and (r.top_set >= 0).all()
    assert sum(len(s) for s in c.sets) > 4096                           # past the first allocation: the buffer grows
