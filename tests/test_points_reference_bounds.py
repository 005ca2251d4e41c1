"""The bounds of the structure-only bundle adjustment tests (points_cases.py) can be met by the reference alone:
the strict CPU oracle against its -ffast-math build, on scenes A and B from start(m, 1), stays inside every bound
and under the 20 % cap on points that end with other counters.  The device differs from the oracle by the same
kind of reordering (FMA contraction, tree sums).  No GPU."""
import pytest

import points_cases as pc


@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_against_itself_first_5_iterations(oracle_lib, name):
    m = pc.started(name)
    points = list(range(m.num_points))
    ref_sums, ref_X = pc.cached_oracle(oracle_lib, name, 5)
    sums, X = pc.cached_oracle(oracle_lib, name, 5, fastmath=True)
    pc.compare_it5("scene %s, fast-math oracle" % name, m, points, sums, X, ref_sums, ref_X)


@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_against_itself_converged(oracle_lib, name):
    m = pc.started(name)
    points = list(range(m.num_points))
    ref_sums, ref_X = pc.cached_oracle(oracle_lib, name, 0)
    sums, X = pc.cached_oracle(oracle_lib, name, 0, fastmath=True)
    pc.compare_converged("scene %s, fast-math oracle" % name, oracle_lib, m, points, sums, X, ref_sums, ref_X)


def test_scenes_are_as_described():
    a, b = pc.scene("A"), pc.scene("B")
    assert (a.num_frames, a.num_points) == (10, 484) and (b.num_frames, b.num_points) == (40, 391)
    ca = [len(pc.enabled_obs(a, p)) for p in range(a.num_points)]
    cb = [len(pc.enabled_obs(b, p)) for p in range(b.num_points)]
    assert (min(ca), max(ca)) == (2, 10) and (min(cb), max(cb)) == (2, 37)
    assert {7, 8, 9, 16, 17, 33} <= set(cb)   # around the lane group of 8 and its multiples
