"""Conditions on the cases of the detector's tests (tests/detect_cases.py) themselves, on the numpy reference and the
oracle's pyramids, so that the equality tests (test_detect_math.py, test_detect_gpu.py) cannot pass on empty ground:
enough keypoints, cells that per_cell cuts and cells it does not, both branches of the two-threshold rule, a tie inside a
cell, candidates on both sides of every cell boundary a planted square straddles, squares exactly at the border and one
pixel outside it.  And the detector's reason to exist: on the 640 x 480 texture the keypoints of frame 0 are found again
in frame 5.

Measured on the oracle's pyramids (printed by the tests):
  candidates at t_lo = 0.01, border 4: 161 x 121 texture 576 / 185 / 45 on its three levels, 96 x 64 texture 165 / 45 / 8;
  at border 15: 412 / 81 / 0 and 73 / 0 / 0 (the small levels are empty there, which is wanted);
  640 x 480 texture, level 0: 7 pairs of equal scores inside one cell among 9911 candidates;
  repeatability frame 0 -> frame 5 at t_lo = t_hi = 7/255, border 15, per_cell 4: 0.731 / 0.787 / 0.770 on levels 0, 1, 2
  (1192 / 287 / 74 keypoints); uniformly random points instead of frame 5's keypoints: 0.029 / 0.035 / 0.054."""
import numpy as np
import pytest

import detect_cases as dc
from slamgpu.video import frame_motion, make_frames


def _cells(r, per_cell):
    """(cells that per_cell cuts, cells with candidates that it does not) of a detect() result."""
    cut = sum(1 for b in r.by_level.values() for v in b["cell_info"].values() if v[1] > per_cell)
    whole = sum(1 for b in r.by_level.values() for v in b["cell_info"].values() if 0 < v[1] <= per_cell)
    return cut, whole


@pytest.mark.parametrize("name", dc.TEXTURE_CASES)
def test_texture_cases_have_keypoints_cut_cells_and_whole_cells(oracle_lib, name):
    pyr = dc.case_levels(name)
    sets = dc.option_sets(pyr)
    res = {on: dc.detect(pyr, **o) for on, o in sets.items()}
    for on, r in res.items():
        print(name, on, len(r.xy), [(p["candidates"], p["low_cells"], p["keypoints"]) for p in r.per_level])
    # at least 50 keypoints: with 16 per cell on both images, and with the default 4 per cell where the image has the
    # cells for it (161 x 121: 24 + 6 + 2 cells; 96 x 64 has 6 + 2 + 1, which 4 per cell limit to 36)
    assert len(res["per_cell16"].xy) >= 50
    if name == "odd":
        assert len(res["border4"].xy) >= 50 and len(res["border15"].xy) >= 50
    # per_cell cuts a cell and leaves another whole, in one call
    cut, whole = _cells(res["per_cell16"], 16)
    assert cut >= 1 and whole >= 1
    cut, whole = _cells(res["median"], 4)
    assert cut >= 1 and whole >= 1
    # every level has candidates at border 4; border 15 empties the small levels and keeps level 0
    assert all(p["candidates"] >= 5 for p in res["border4"].per_level)
    assert res["border15"].per_level[0]["candidates"] >= 50 and res["border15"].per_level[-1]["candidates"] == 0
    # the caps: one cuts, one does not, and the cut reaches across levels
    assert len(res["cap_half"].xy) == sets["cap_half"]["max_keypoints"] < len(res["border4"].xy)
    assert len(res["cap_equal"].xy) == len(res["border4"].xy)
    assert len(set(res["cap_half"].levels)) >= 2
    assert len(res["level1"].xy) >= 5 and set(res["level1"].levels) == {1}


def test_median_threshold_puts_cells_on_both_branches(oracle_lib):
    pyr = dc.case_levels("odd")
    r = dc.detect(pyr, **dc.option_sets(pyr)["median"])
    info = r.by_level[0]["cell_info"]
    low = r.per_level[0]["low_cells"]
    high = len(info) - low
    print("median case, level 0: cells with candidates %d, low %d, high %d" % (len(info), low, high))
    assert low >= 5 and high >= 5
    # and the high branch drops candidates: a cell where fewer are eligible than there are
    assert any(v[1] < v[0] for v in info.values())


def test_planted_squares_tie_straddle_the_cells_and_probe_the_border(oracle_lib):
    pyr = dc.case_levels("planted")
    found = {}
    for border in (4, 15):
        x, y, s = dc.detect_level(pyr[0], dc.T_LO, dc.T_HI, border, 4)["cand"]
        found[border] = {(int(a), int(b)): float(c) for a, b, c in zip(x, y, s)}
        # every planted square whose centre is admissible is a candidate at its centre, and no other pixel is one
        want = {(px, py) for px, py, _ in dc.PLANTED
                if border <= px <= dc.PLANT_W - 1 - border and border <= py <= dc.PLANT_H - 1 - border}
        assert set(found[border]) == want, border
    # the squares exactly at the border are in, those a pixel further out are not
    at = found[4]
    assert (4, 4) in at and (92, 65) in at and not {(3, 58), (93, 8), (80, 3), (80, 66)} & set(at)
    assert (15, 15) in found[15] and (81, 54) in found[15]
    assert not {(14, 46), (82, 40), (47, 14), (66, 55)} & set(found[15])
    # a tie inside a cell: the two equal squares of cell (1, 1)
    assert at[(40, 46)] == at[(54, 46)] and 40 // 32 == 54 // 32
    # a candidate on both sides of each straddled boundary
    for axis, a, b in dc.STRADDLED:
        k = 0 if axis == "x" else 1
        assert any(p[k] == a for p in at) and any(p[k] == b for p in at), (axis, a, b)
    assert (31, 31) in at and (64, 32) in at
    # the tie is decided by the pixel index: cell (1, 1) holds the dark square (47, 32), which scores higher, and the
    # two equal bright ones; with two keypoints per cell the first of the pair gets the second place
    r = dc.detect(pyr, per_cell=2, first_level=0, num_levels=1)
    kept = set(zip(r.x.tolist(), r.y.tolist()))
    assert at[(47, 32)] > at[(40, 46)] and {(47, 32), (40, 46)} <= kept and (54, 46) not in kept


def test_constant_and_thin_images(oracle_lib):
    pyr = dc.case_levels("constant")
    assert len(dc.detect(pyr).xy) == 0 and all(p["candidates"] == 0 for p in dc.detect(pyr).per_level)
    pyr = dc.case_levels("thin")
    r = dc.detect(pyr)
    assert [(p["width"], p["height"], p["cells"]) for p in r.per_level] == [(33, 9, 2), (17, 5, 1)]
    assert len(r.xy) >= 1 and (r.y == 4).all() and (r.x < 32).all()      # the one admissible row, the first cell only
    assert len(dc.detect(pyr, border=15).xy) == 0


@pytest.fixture(scope="module")
def frames():
    return make_frames(6)


def test_texture_level_holds_equal_scores_inside_a_cell(oracle_lib, frames):
    r = dc.detect_level(dc.oracle_levels(frames[0], 1)[0], dc.T_LO, dc.T_HI, 4, 4)
    x, y, s = r["cand"]
    cell = (y // dc.CELL) * ((r["w"] + dc.CELL - 1) // dc.CELL) + x // dc.CELL
    pairs = sum(int((cell == c).sum()) - len(np.unique(s[cell == c])) for c in np.unique(cell))
    print("640 x 480 texture, level 0: %d candidates, %d pairs of equal scores inside a cell" % (len(x), pairs))
    assert pairs >= 1


def test_keypoints_of_frame_0_are_found_again_in_frame_5(oracle_lib, frames):
    """Share of frame-0 keypoints that land inside frame 5 and have a frame-5 keypoint of the same level within
    1.5 * 2^l px of where frame_motion puts them: at least 0.6 on every level."""
    t = np.float32(7.0 / 255.0)
    a, b = (dc.detect(dc.oracle_levels(frames[f], 3), threshold=t, min_threshold=t, border=15, per_cell=4)
            for f in (0, 5))
    R, d, ctr = frame_motion(5)
    rng = np.random.default_rng(7)
    for l in range(3):
        pa, pb = a.xy[a.levels == l].astype(np.float64), b.xy[b.levels == l].astype(np.float64)
        m = (pa - ctr) @ R.T + ctr + d
        m = m[(m[:, 0] >= 0) & (m[:, 0] <= 639) & (m[:, 1] >= 0) & (m[:, 1] <= 479)]
        near = lambda q: float((np.sqrt(((m[:, None, :] - q[None]) ** 2).sum(-1)).min(1) <= 1.5 * 2 ** l).mean())  # noqa: E731
        share = near(pb)
        chance = near(rng.uniform([15 * 2 ** l, 15 * 2 ** l], [640 - 15 * 2 ** l, 480 - 15 * 2 ** l], pb.shape))
        print("level %d: %d keypoints, %d inside frame 5, repeatability %.3f, random points %.3f"
              % (l, len(pa), len(m), share, chance))
        assert len(m) >= 50
        assert share >= 0.6
        assert chance <= 0.15      # the density of the points alone does not explain it
