"""Conditions on the inputs of the epipolar matching tests, and proof that the planted items bite (numpy only, no
library, no GPU).

The GPU test compares integers with the numpy reference exactly.  That is sound only when no decision of the contract
sits within rounding of its threshold: the device may contract a product and a sum into one fused operation where
numpy rounds twice, sums dot products in another order, and has its own atan2.  Those differences are a few ulp
(1e-16 relative) of the largest term of each expression, so every decision that is reached must stay NEAR = 1e-9
away from its threshold relative to that term: the gate |r^2 - tol^2 4^L den| against tol^2 4^L den; det against
(g.g)(f.f); each depth numerator against the sum of the magnitudes of its two products; the parallax against
min_parallax.

Measured on the reference (seeds as committed): on the four c1 cases every true pair is a candidate of its keypoint
where no parallax is asked for.  Of the true pairs, match recovers 1.000 (c1, c1_levels) and 0.492 (c1_parallax,
c1_levels_parallax: the forward-moving pairs (0,2) and (1,3) have little parallax); of the accepted matches, 1.000 are
true in all four.  Smallest margins seen: gate 2.5e-6, det 2.0e-8, depth 2.4e-7, parallax 7.1e-4."""
import numpy as np
import pytest

import epipolar_cases as ec

RECALL = {"c1": 1.000, "c1_levels": 1.000, "c1_parallax": 0.492, "c1_levels_parallax": 0.492}
PRECISION = {"c1": 1.000, "c1_levels": 1.000, "c1_parallax": 1.000, "c1_levels_parallax": 1.000}
SLACK = 0.05     # lets a change of seed pass; the device is judged by equality, not by these


@pytest.mark.parametrize("name", ec.CASE_NAMES)
def test_no_input_sits_on_a_decision(name):
    for p, r in zip(ec.case(name).pairs, ec.expected(name)):
        nc, g = r["num_candidates"], r["gaps"]
        print("%s pair %s: %d x %d keypoints, candidates mean %.2f max %d, none %d, one %d; margins: gate %.3e, det %.3e,"
              " depth %.3e, parallax %.3e" % (name, p, r["num_a"], r["num_b"], nc.mean() if len(nc) else 0.0,
                                              nc.max() if len(nc) else 0, int((nc == 0).sum()), int((nc == 1).sum()),
                                              g["gate"], g["det"], g["depth"], g["parallax"]))
        for k in ("gate", "det", "depth", "parallax"):
            assert g[k] > ec.NEAR, (name, p, k, g[k])


def test_generated_cases_reach_every_path():
    c1 = ec.expected("c1")
    # every c1 pair takes several chunks of a keypoints and ends on a partial one; the gate leaves a few candidates
    assert all(r["num_a"] > 2 * ec.CHUNK and r["num_a"] % ec.CHUNK and r["num_b"] > ec.TILE for r in c1)
    assert all(1.0 < r["num_candidates"].mean() < 10.0 for r in c1)
    # levels widen the gate; the parallax test removes candidates; both cameras are in use
    assert all(b["num_candidates"].sum() > a["num_candidates"].sum() for a, b in zip(c1, ec.expected("c1_levels")))
    assert all(b["num_candidates"].sum() < a["num_candidates"].sum() for a, b in zip(c1, ec.expected("c1_parallax")))
    m = ec.case("c1").m
    assert m.frame_camera[0] != m.frame_camera[1] and not np.array_equal(m.k[:7], m.k[7:14])
    # the depth test is felt: it cuts the candidates of the gate alone
    gate_only = ec.reference(ec.case("c1"), off=("depth",))
    assert all(b["num_candidates"].sum() > 1.5 * a["num_candidates"].sum() for a, b in zip(c1, gate_only))
    # shapes: every (na, nb), windows of tens of candidates, ties for best in plenty, all three slice counts
    sh, want = ec.case("shapes"), ec.expected("shapes")
    assert sorted((r["num_a"], r["num_b"]) for r in want) == sorted((a, b) for a in ec.NA for b in ec.NB)
    assert len(set(sh.pairs)) == 1
    allc = np.concatenate([r["num_candidates"] for r in want])
    tied = np.concatenate([(r["best_dist"] == r["second_dist"]) & (r["best_dist"] >= 0) for r in want])
    assert allc.max() > 100 and tied.sum() > 100
    assert {-(-nb // ec.SLICE) for nb in ec.NB} == {1, 2, 3}
    assert ec.SLICE % ec.TILE == 0 and any(nb % ec.TILE % 4 for nb in ec.NB)


@pytest.mark.parametrize("name", ["c1", "c1_levels", "c1_parallax", "c1_levels_parallax"])
def test_true_pairs_on_exact_poses(name):
    c, want = ec.case(name), ec.expected(name)
    true = cand = hit = accepted = 0
    for (fa, fb), r, t in zip(c.pairs, want, c.truth):
        assert len(t.ia) >= 10
        is_cand = r["cand"][t.ia, t.jb]
        if c.options["min_parallax"] == 0:
            assert is_cand.all(), (name, fa, fb)            # exact: the poses and the pixels are the scene's own
        else:
            # the true pairs that are missing are those whose rays meet at less than min_parallax, by the scene's
            # geometry alone: the angle at the landmark between the two camera centres
            X = c.m.X_true.reshape(-1, 4)[t.point]
            X = X[:, :3] / X[:, 3:]
            u, v = X - c.m.t[3 * fa:3 * fa + 3], X - c.m.t[3 * fb:3 * fb + 3]
            angle = np.arctan2(np.linalg.norm(np.cross(u, v), axis=1), (u * v).sum(1))
            assert np.array_equal(is_cand, angle >= c.options["min_parallax"]), (name, fa, fb)
        true += len(t.ia)
        cand += int(is_cand.sum())
        hit += int((r["match"][t.ia] == t.jb).sum())
        accepted += r["num_matched"]
    recall, precision = hit / true, hit / accepted
    print("%s: %d true pairs, %d candidates, %d recovered of %d accepted: recall %.3f precision %.3f" % (
        name, true, cand, hit, accepted, recall, precision))
    assert recall >= RECALL[name] - SLACK and precision >= PRECISION[name] - SLACK


def _row(r, names, name):
    i = names.index(name)
    return tuple(int(r[a][i]) for a in ec.ARRAYS)


def test_planted_items_give_what_they_were_planted_for():
    c = ec.case("planted")
    full, plain = ec.expected("planted"), ec.expected("planted_plain")
    a, b = c.a_names, c.b_names
    on, off = full[0], plain[0]
    j = {n: i for i, n in enumerate(b)}
    empty = (-1, -1, -1, -1, 0)
    for r in (on, off):
        # the same descriptor twice on one line: the lower index wins and second == best
        assert j["tie_lo"] < j["tie_hi"] and _row(r, a, "tie") == (j["tie_lo"], j["tie_lo"], 0, 0, 2)
        assert _row(r, a, "alike") == (-1, j["alike_a"], 20, 24, 2)               # 2000 > 80 * 24
        # two a keypoints claim one b keypoint: the nearer descriptor wins
        assert _row(r, a, "claim_far") == (-1, j["shared"], 5, -1, 1) and _row(r, a, "claim_near")[0] == j["shared"]
        assert _row(r, a, "behind") == empty                                      # on the line, behind both cameras
        assert _row(r, a, "nan_x") == _row(r, a, "inf_y") == _row(r, a, "empty") == empty
        assert _row(r, a, "single") == (j["single"], j["single"], 7, -1, 1)
        assert _row(r, a, "too_far") == (-1, j["too_far"], 70, -1, 1)
        assert not r["cand"][:, j["nan_y"]].any()
    # refused only by parallax, admitted only through the level of b, and of a
    assert _row(on, a, "flat") == empty and _row(off, a, "flat") == (j["flat"], j["flat"], 2, -1, 1)
    assert _row(on, a, "level_b") == (j["level_b"], j["level_b"], 2, -1, 1) and _row(off, a, "level_b") == empty
    assert _row(on, a, "level_a") == (j["level_a"], j["level_a"], 2, -1, 1) and _row(off, a, "level_a") == empty
    # the zero-baseline pair is degenerate and empty; the pair without a keypoints is empty, not degenerate
    for r in (full, plain):
        assert r[1]["degenerate"] == 1 and r[1]["num_matched"] == 0 and (r[1]["num_candidates"] == 0).all()
        assert (r[1]["num_a"], r[1]["num_b"]) == (len(a), len(b))
        assert [r[3][k] for k in ec.COUNTS] == [0, 3, 0, 0, 0]
        assert [r[i]["degenerate"] for i in (0, 2)] == [0, 0]
    # the planted pair listed again with the first five a keypoints and the b keypoints reversed
    again, nb = full[2], len(b)
    for i in range(5):
        first = _row(on, a, a[i])
        want = tuple(nb - 1 - v if k < 2 and v >= 0 else v for k, v in enumerate(first))
        if a[i] == "tie":      # reversing b swaps which of the equal descriptors has the lower index
            want = (nb - 1 - j["tie_hi"], nb - 1 - j["tie_hi"], 0, 0, 2)
        assert _row(again, a, a[i]) == want, a[i]


@pytest.mark.parametrize("rule, keypoint", [("tie", "tie"), ("ratio", "alike"), ("unique", "claim_far"),
                                            ("depth", "behind"), ("parallax", "flat"), ("level", "level_b"),
                                            ("level", "level_a")])
def test_each_planted_item_bites(rule, keypoint):
    c = ec.case("planted")
    want, without = ec.expected("planted")[0], ec.reference(c, off=(rule,))[0]
    i = c.a_names.index(keypoint)
    assert want["match"][i] != without["match"][i], (rule, want["match"][i])
    others = [k for k in range(len(c.a_names)) if k != i and not (rule == "level" and c.a_names[k].startswith("level"))]
    assert np.array_equal(want["match"][others], without["match"][others])
