"""The bounds of the triangulation tests (triangulate_cases.py) from the reference alone: the numpy restatement
with each point's records summed forward against reversed (c0 and L kept), on scenes A and B, noisy and exact.  The
worst differences are printed and must stay within the SPREAD_* values; the device tests allow 100 x those.  Also
checks what the device tests rely on: the exact scenes triangulate to the truth, both gated statuses occur on the
noisy scenes and no point sits within 1e-6 of a gate.  No GPU."""
import numpy as np
import pytest

import triangulate_cases as tc


@pytest.mark.parametrize("exact", [False, True], ids=["noisy", "exact"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_forward_against_reversed(name, exact):
    fwd = tc.reference(name, exact)
    rev = tc.reference(name, exact, reverse=True)
    assert [r["status"] for r in fwd] == [r["status"] for r in rev]
    tc.compare("scene %s %s, reversed sums" % (name, "exact" if exact else "noisy"), rev, fwd, margin=1.0)


@pytest.mark.parametrize("name", ["A", "B"])
def test_exact_scenes_triangulate_to_the_truth(name):
    m = tc.scene(name, exact=True)
    ref = tc.reference(name, exact=True)
    assert all(r["status"] == "OK" for r in ref)
    err = max(r["max_error_px"] for r in ref)
    truth = [dict(r, X=m.X_true[4 * p:4 * p + 4]) for p, r in enumerate(ref)]
    print("scene %s exact: worst max_error_px %.2e" % (name, err))
    assert err <= tc.EXACT_ERROR_PX
    w = tc.spreads(ref, truth)
    print("scene %s exact against X_true: |dX| rel_gap %.2e; |dX| %.2e" % (name, w["x_gap"], w["x"]))
    assert w["x_gap"] <= tc.MARGIN * tc.SPREAD_X_GAP and w["x"] <= tc.MARGIN * tc.SPREAD_X


def test_gated_statuses_occur_and_no_point_is_near_a_gate():
    over, under = [], []
    for name in ("A", "B"):
        ref = tc.reference(name, gates=True)
        st = [r["status"] for r in ref]
        over.append(st.count("HIGH_ERROR"))
        under.append(st.count("LOW_PARALLAX"))
        print("scene %s: %s" % (name, {k: st.count(k) for k in sorted(set(st))}))
        d_px = min(abs(r["max_error_px"] - tc.GATE_PX) for r in ref)
        d_rad = min(abs(r["parallax"] - tc.GATE_RAD) for r in ref)
        print("scene %s: nearest to the gates %.3f px, %.4f deg" % (name, d_px, np.rad2deg(d_rad)))
        assert d_px > tc.NEAR_GATE and d_rad > tc.NEAR_GATE
    print("over 5 px: %s; under 1 deg: %s" % (over, under))
    assert min(over) > 0 and min(under) > 0


def test_scenes_are_as_described():
    a, b = tc.scene("A"), tc.scene("B")
    assert (a.num_points, b.num_points) == (484, 391)
    assert (tc.scene("A", True).num_points, tc.scene("B", True).num_points) == (484, 391)
    assert a.q.tobytes() == a.q_true.tobytes() and b.t.tobytes() == b.t_true.tobytes()
