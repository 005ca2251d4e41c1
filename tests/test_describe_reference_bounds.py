"""The numpy reference of sg_tracker_describe (tests/describe_cases.py) on its own: the cases stay non-trivial and
decidable, and the descriptor it defines does what an oriented descriptor is for.  No GPU, none of the library's code.

Cases: every keypoint the reference accepts has a gap of 1e-9 or more (so the exact comparisons of
test_describe_math.py and test_describe_gpu.py have one right answer each), every bin occurs, every border side refuses
a keypoint and accepts its neighbour one pixel inside, and about half the bits of a descriptor are set.

Properties: a quarter turn of the level turns every bin by a quarter turn and leaves every descriptor as it was;
frame 0 of the texture matches its own rotation by 10, 37 and 80 degrees; without the steering the 37 degree case
collapses, so that case exercises the steering."""
import numpy as np
import pytest

import describe_cases as dc

# nearest-neighbour share measured by this reference on the oracle pyramid (0.956, 0.938, 0.961 on 547, 481 and 439
# keypoints; true pairs 29 to 33 bits apart on average, the best wrong candidate 63 to 64), rounded down to the
# next 0.05
ROTATION_FLOOR = {10: 0.95, 37: 0.90, 80: 0.95}


@pytest.mark.parametrize("name", list(dc.DEVICE_CASES))
def test_device_cases_are_decidable_and_probe_every_border(oracle_lib, name):
    c, e = dc.device_case(name), dc.device_expected(name)
    ok = e["status"] == 0
    assert len(c.xy) == dc.N_DEVICE and ok.sum() >= 100 and (~ok).sum() >= 30
    print(name, "accepted", ok.sum(), "smallest gap", e["gap"][ok].min())
    assert (e["gap"][ok] >= dc.GAP).all(), e["gap"][ok].min()
    assert (e["angle_bin"][~ok] == -1).all() and not e["desc"][~ok].any()
    for l in range(c.depth):
        wl, hl = dc.pyramid_dims(c.w, c.h, c.depth)[l]
        on = c.levels == l
        for s in range(4):
            out, ins = on & (c.side == s) & (c.inside == 0), on & (c.side == s) & (c.inside == 1)
            assert out.any() and ins.any()
            assert (e["status"][out] == 1).all(), (name, l, dc.SIDES[s])
            if wl >= 31 and hl >= 31:      # one pixel inside the side: accepted
                assert (e["status"][ins] == 0).any(), (name, l, dc.SIDES[s])
            else:                          # a level smaller than 31 refuses everything
                assert (e["status"][on] == 1).all()
    # the special keypoints are there: non-finite coordinates, coordinates ending in .5, a level below 31 (one case)
    assert (~np.isfinite(c.xy).all(1)).sum() >= 5 and (e["status"][~np.isfinite(c.xy).all(1)] == 1).all()
    with np.errstate(invalid="ignore"):
        half = ok & ((c.xy * np.float32(0.5) ** c.levels[:, None] % 1.0) == 0.5).any(1)
    assert half.sum() >= 2
    # the small calls of the GPU test are prefixes: levels and both answers mixed early on
    assert len(set(c.levels[:5])) >= 2


def test_one_device_case_has_a_level_below_31_and_one_a_single_row():
    dims = {nm: dc.pyramid_dims(*dc.DEVICE_CASES[nm]) for nm in dc.DEVICE_CASES}
    assert dims["odd"] == [(161, 121), (81, 61), (41, 31)] and dims["stride"][2] == (24, 16)
    assert dc.device_case("stride").img.strides[0] > 3 * 96


def test_texture_case_gaps_bins_and_bit_balance(oracle_lib):
    e = dc.texture_expected(all_level0=True)
    assert (e["status"] == 0).all() and len(e["status"]) == 600
    print("smallest gap over 600 seed points", e["gap"].min())
    assert (e["gap"] >= dc.GAP).all()
    assert sorted(set(e["angle_bin"])) == list(range(32))
    bits = dc.popcount(e["desc"])
    assert 96 <= bits.mean() <= 160, bits.mean()
    m = dc.texture_expected()      # the same points on levels 0, 1, 2
    ok = m["status"] == 0
    assert ok.sum() > 400 and (m["gap"][ok] >= dc.GAP).all() and 96 <= dc.popcount(m["desc"][ok]).mean() <= 160
    for name in dc.DEVICE_CASES:
        d = dc.device_expected(name)
        assert 96 <= dc.popcount(d["desc"][d["status"] == 0]).mean() <= 160
    # distinct keypoints get distinct descriptors: wrong pairs are far apart
    d = dc.hamming(e["desc"][:200], e["desc"][:200])
    assert d[~np.eye(200, dtype=bool)].mean() > 100


def test_quarter_turn_of_the_level_turns_the_bin_and_keeps_the_descriptor(oracle_lib):
    c = dc.texture_case()
    lv = c.pyr[0]
    h, w = lv.shape
    a = dc.reference_level(lv, c.xy)
    cx, cy, ok = dc.centres(c.xy, 0, w, h)
    assert ok.all()
    # np.rot90: pixel (x, y) of the level lands on (y, w - 1 - x); offsets (u, v) become (v, -u), a quarter turn back
    turned = np.ascontiguousarray(np.rot90(lv))
    b = dc.reference_level(turned, np.stack([cy, w - 1 - cx], 1).astype(np.float32))
    assert (b["status"] == 0).all() and (b["gap"] >= dc.GAP).all()
    np.testing.assert_array_equal(b["angle_bin"], (a["angle_bin"] - 8) % 32)
    np.testing.assert_array_equal(b["desc"], a["desc"])
    scale = np.hypot(a["m10"], a["m01"])                  # the same products summed in another order
    assert (np.abs(b["m10"] - a["m01"]) <= 1e-12 * scale).all() and (np.abs(b["m01"] + a["m10"]) <= 1e-12 * scale).all()


@pytest.mark.parametrize("deg", sorted(ROTATION_FLOOR))
def test_rotated_frame_matches_itself(oracle_lib, deg):
    """Floors 0.95 / 0.90 / 0.95 at 10 / 37 / 80 degrees: the shares this reference measures on the oracle pyramid
    (0.956 of 547 keypoints, 0.938 of 481, 0.961 of 439), rounded down to the next 0.05."""
    share, n, own, wrong = dc.rotation_match(deg)
    print("rotation %d: share %.4f on %d keypoints, true pairs %.1f bits, best wrong %.1f" % (deg, share, n, own, wrong))
    assert n >= 400
    assert share >= ROTATION_FLOOR[deg], share
    assert own < wrong


def test_without_steering_the_37_degree_case_collapses(oracle_lib):
    share, n, own, _ = dc.rotation_match(37, steer=False)
    print("unsteered 37: share %.4f on %d keypoints, true pairs %.1f bits" % (share, n, own))
    assert share < 0.5 * ROTATION_FLOOR[37], share
