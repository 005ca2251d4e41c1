"""Conditions on the inputs of the match-by-projection tests, and proof that the planted cases bite (numpy only, no
library, no GPU).

The GPU tests compare integers with the numpy reference exactly.  That is sound only when no decision of the contract
sits within rounding of its threshold: the device may contract a product and a sum of Project into one fused operation
where numpy rounds twice, which moves a projection by a few ulp of a pixel (about 1e-13 px).  So, on every case, with
cap 0 (no exception allowed):
  * no keypoint-survivor distance lies within NEAR = 1e-6 px of the radius;
  * no projection lies within NEAR of an image border (where a bound is given);
  * no p.z lies within 1e-9 relative of the 0.001 W refusal line.
Each planted case must change the reference answer when the rule it targets is switched off in the reference."""
import numpy as np
import pytest

import match_cases as mc


@pytest.mark.parametrize("name", mc.CASE_NAMES)
def test_no_input_sits_on_a_decision(name):
    for f, r in zip(mc.case(name).frames, mc.expected(name)):
        nc = r["num_candidates"]
        print("%s frame %d: %d keypoints, %d survivors, window mean %.2f max %d, empty %d, single %d; gaps: radius %.3e px,"
              " border %.3e px, z %.3e" % (name, f, r["num_keypoints"], r["num_projected"], nc.mean() if len(nc) else 0.0,
                                           nc.max() if len(nc) else 0, int((nc == 0).sum()), int((nc == 1).sum()),
                                           r["radius_gap"], r["border_gap"], r["z_gap"]))
        assert r["radius_gap"] > mc.NEAR
        assert r["border_gap"] > mc.NEAR
        assert r["z_gap"] > mc.NEAR_Z


def test_generated_cases_reach_every_path():
    c1, lg = mc.expected("c1"), mc.expected("long")
    # both frames of C1 take several keypoint chunks and end on a partial one
    assert all(r["num_keypoints"] > 2 * mc.CHUNK and r["num_keypoints"] % mc.CHUNK for r in c1)
    # skip_observed removes some but not all of the map's points there
    off = mc.expected("c1_skip_off")
    assert all(0 < a["num_projected"] < b["num_projected"] for a, b in zip(c1, off))
    # the long case: several survivor slices with a partial last one and a partial last tile, many chunks
    for r in lg:
        assert r["num_projected"] > 4 * mc.SLICE and r["num_projected"] % mc.SLICE and r["num_projected"] % 256
        assert r["num_keypoints"] > 8 * mc.CHUNK and r["num_candidates"].mean() > 5
        assert (r["num_candidates"] == 1).any() and (r["num_candidates"] == 0).any()
    # the bounded case culls points that would otherwise project, and both cameras are in use
    assert any(a["num_projected"] < 484 for a in mc.expected("c1_bounded"))
    m = mc.case("c1").m
    assert m.frame_camera[3] != m.frame_camera[8] and not np.array_equal(m.k[:7], m.k[7:14])
    # no point is refused behind the camera in the generated scenes: that rule is planted
    assert all(r["num_projected"] == 484 for r in off)


def test_planted_cases_give_what_they_were_planted_for():
    c = mc.case("planted_skip_on")
    e = {k: mc.expected("planted_" + k)[0] for k in ("skip_on", "skip_off", "obs_disabled", "bounded")}
    kp = {n: i for i, n in enumerate(c.kp_names)}
    idx = c.idx
    on = e["skip_on"]

    def row(r, name):
        i = kp[name]
        return tuple(int(r[a][i]) for a in ("match", "best_point", "best_dist", "second_dist", "num_candidates"))

    assert len(c.points) == 13 and on["num_projected"] == 10          # behind, NaN and the observed point are out
    assert e["skip_off"]["num_projected"] == e["obs_disabled"]["num_projected"] == 11
    assert e["bounded"]["num_projected"] == 9                          # and the point left of the image
    assert row(on, "at_behind") == row(on, "empty") == row(on, "nan_x") == row(on, "inf_y") == (-1, -1, -1, -1, 0)
    assert row(on, "at_left") == (idx["left"], idx["left"], 2, -1, 1)
    assert row(e["bounded"], "at_left") == (-1, -1, -1, -1, 0)
    assert row(on, "single") == (idx["single"], idx["single"], 7, -1, 1)
    # the same descriptor twice: the lower position wins, which here is the higher map index, and second == best
    assert list(c.points).index(idx["tie_lo"]) < list(c.points).index(idx["tie_hi"]) and idx["tie_lo"] > idx["tie_hi"]
    assert row(on, "tie") == (idx["tie_lo"], idx["tie_lo"], 0, 0, 2)
    assert row(on, "tie_flipped") == (-1, idx["tie_lo"], 3, 3, 2)      # a tie above zero fails the ratio test
    # the observed point is the nearest descriptor: skipped, taken, and taken again once its observation is disabled
    assert row(on, "near_seen") == (idx["unseen"], idx["unseen"], 40, -1, 1)
    assert row(e["skip_off"], "near_seen") == row(e["obs_disabled"], "near_seen") == (idx["seen"], idx["seen"], 2, 40, 2)
    # two keypoints claim one point: the nearer descriptor wins; at equal distance the lower keypoint index
    assert row(on, "claim_far") == (-1, idx["shared"], 5, -1, 1) and row(on, "claim_near")[0] == idx["shared"]
    assert kp["claim_eq_first"] < kp["claim_eq_second"]
    assert row(on, "claim_eq_first")[0] == idx["shared_eq"] and row(on, "claim_eq_second") == (-1, idx["shared_eq"], 4, -1, 1)
    assert row(on, "alike") == (-1, idx["alike_a"], 20, 24, 2)         # 2000 > 80 * 24
    assert row(on, "far")[0] == idx["far"] and row(on, "too_far") == (-1, idx["far"], 70, -1, 1)
    # a frame without keypoints still counts its candidates
    assert mc.expected("planted_skip_on")[1]["num_keypoints"] == 0 and mc.expected("planted_skip_on")[1]["num_projected"] > 0


@pytest.mark.parametrize("rule, name, keypoint", [("exclusion", "planted_skip_on", "near_seen"),
                                                  ("bounds", "planted_bounded", "at_left"),
                                                  ("tie", "planted_skip_on", "tie"),
                                                  ("ratio", "planted_skip_on", "alike"),
                                                  ("unique", "planted_skip_on", "claim_far")])
def test_each_planted_case_bites(rule, name, keypoint):
    c = mc.case(name)
    want, without = mc.expected(name)[0], mc.reference(c, off=(rule,))[0]
    i = c.kp_names.index(keypoint)
    assert want["match"][i] != without["match"][i], (rule, want["match"][i])
    # the generated scenes feel the exclusion too (their random descriptors neither tie for best, nor come close enough
    # to fail the ratio test, nor draw two keypoints to one point: those rules rest on the planted cases)
    if rule == "exclusion":
        a, b = mc.expected("c1"), mc.reference(mc.case("c1"), off=(rule,))
        assert all(not np.array_equal(x["match"], y["match"]) for x, y in zip(a, b))
