"""The bounds of the reduced-system shape tests (ba_shape_cases.py) can be met by the reference alone.  On every
case of the size, band and path sweeps the CPU oracle takes 3 successful LM steps and none rejected, which is what an
iteration-for-iteration comparison needs, and it differs from itself (1 thread against 4 threads, and against its
-ffast-math build) by at most half of each bound.  The device differs from the oracle by the same kind of reordering
(FMA contraction, tree and tile sums).  No GPU."""
import pytest

import ba_shape_cases as bc

GROUPS = {
    "size_1_16": [c for c in bc.SIZE_SWEEP if c[0] <= 16],
    "size_17_32": [c for c in bc.SIZE_SWEEP if 16 < c[0] <= 32],
    "size_33_48": [c for c in bc.SIZE_SWEEP if c[0] > 32],
    "band_35": [c for c in bc.BAND_SWEEP if c[0] == 35],
    "band_46": [c for c in bc.BAND_SWEEP if c[0] == 46],
}


def test_cases_are_as_described():
    assert {bc.tile_rows(6 * solve) for solve, _ in bc.SIZE_SWEEP} == set(range(1, 19))
    assert {16 * bc.tile_rows(6 * solve) - 6 * solve for solve, _ in bc.SIZE_SWEEP} == set(range(0, 16, 2))
    assert all(r != 2 for _, r in bc.SIZE_SWEEP + bc.BAND_SWEEP)
    assert len(bc.BAND_SPLIT) == 16
    # the path sweep forces kernels on problems of the other two sweeps: the groups below cover it
    assert {(solve, r) for solve, r, _, _ in bc.PATH_SWEEP} <= set(bc.SIZE_SWEEP + bc.BAND_SWEEP)
    assert sorted(c for g in GROUPS.values() for c in g) == sorted(bc.SIZE_SWEEP + bc.BAND_SWEEP)
    for solve, r in ((1, 14), (35, 3), (46, 26)):
        pa = bc.problem(solve, r)
        free = pa.frame_rot_free.astype(bool) | pa.frame_trans_free.astype(bool)
        assert int(free.sum()) == solve and pa.num_frames == solve + 2


@pytest.mark.parametrize("group", list(GROUPS))
def test_reference_against_itself(oracle_lib, group):
    results = {"4 threads": [], "fast-math": []}
    for solve, r in GROUPS[group]:
        name = "solve=%d r=%d" % (solve, r)
        rs, rp = bc.oracle_result(oracle_lib, solve, r)
        assert rs["ok"] == 1 and rs["num_successful_steps"] == bc.ITERATIONS, (name, rs)
        assert rs["num_unsuccessful_steps"] == 0 and rs["num_invalid_steps"] == 0, (name, rs)
        assert rs["num_iterations"] == bc.ITERATIONS + 1, (name, rs)
        s4, p4 = bc.oracle_result(oracle_lib, solve, r, nthreads=4)
        sf, pf = bc.oracle_result(oracle_lib, solve, r, fastmath=True)
        results["4 threads"].append((name, s4, p4, rs, rp))
        results["fast-math"].append((name, sf, pf, rs, rp))
    for other, rows in results.items():
        bc.compare("%s, oracle with %s against the oracle" % (group, other), "reference alone", rows, share=0.5)
