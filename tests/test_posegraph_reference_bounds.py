"""The numpy reference of the pose-graph tests (tests/posegraph_cases.py) held to its own conditions, on the CPU, so
that the device tests cannot hide a failure: its analytic Jacobian against central differences; its rounding floor
(SPREAD: listed against reversed order) recomputed and compared with the written constants, each of which must be an
upper bound within a factor of 4; and the conditions under which iteration counts can be compared exactly.  No GPU, no
library."""
import numpy as np
import pytest

import posegraph_cases as pc


def _random_state(rng, sigma=True):
    x = np.zeros(8)
    x[:4] = pc.qunit(rng.normal(size=4))
    x[4:7] = rng.normal(0.0, 500.0, size=3)
    x[7] = rng.normal(0.0, 0.2) if sigma else 0.0
    return x


def _numeric_jacobian(xa, xb, meas, w, fs, h=1e-6):
    D = 6 if fs else 7
    J = np.zeros((7, 14))
    for side in (0, 1):
        for k in range(D):
            d = np.zeros(7)
            d[k] = h
            pa, ma = (pc.node_plus(xa, d, fs), pc.node_plus(xa, -d, fs)) if side == 0 else (xa, xa)
            pb, mb = (pc.node_plus(xb, d, fs), pc.node_plus(xb, -d, fs)) if side == 1 else (xb, xb)
            J[:, 7 * side + k] = (pc.edge_residual(pa, pb, meas, w, fs) - pc.edge_residual(ma, mb, meas, w, fs)) / (2 * h)
    return J


@pytest.mark.parametrize("kind", ["random", "series_below", "series_above", "flip_plus", "flip_minus"])
@pytest.mark.parametrize("fs", [False, True])
def test_reference_jacobian_matches_central_differences(kind, fs):
    rng = np.random.default_rng(5)
    w = np.array([3.0, 0.7, 11.0])
    for _ in range(5):
        xa, xb = _random_state(rng, not fs), _random_state(rng, not fs)
        qrel = pc.qmul(xa[:4], pc.qconj(xb[:4]))
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        # q_e = conj(q^) (x) qrel is the rotation by `ang` about ax
        ang = {"random": rng.uniform(0.3, 2.5), "series_below": 1.6e-4, "series_above": 2.4e-4,
               "flip_plus": np.pi - 1e-3, "flip_minus": np.pi + 1e-3}[kind]
        qe = np.concatenate([np.sin(ang / 2) * ax, [np.cos(ang / 2)]])
        qh = pc.qmul(qrel, pc.qconj(qe))
        meas = np.concatenate([qh / np.linalg.norm(qh), rng.normal(0.0, 300.0, size=3), [0.1]])
        J = pc.edge_jacobian(xa, xb, meas, w, fs)
        Jn = _numeric_jacobian(xa, xb, meas, w, fs)
        # central differences with h = 1e-6 on values of a few thousand: 1e-6 of the largest entry
        assert np.abs(J - Jn).max() <= 2e-6 * max(1.0, np.abs(Jn).max()), (kind, np.abs(J - Jn).max())


@pytest.mark.parametrize("name", pc.SCENES)
def test_spread_constants_are_tight_upper_bounds(name):
    sc = pc.scene(name)
    ref = pc.reference(name)
    rev = pc.solve_np(pc.reversed_scene(sc), pc.SCENE_OPTIONS.get(name))
    got = pc.compare(ref["x"], rev["x"][::-1])
    got["cost"] = abs(ref["final_cost"] - rev["final_cost"])
    print(name, got, "cost floor %.3g" % pc.cost_floor(sc))
    for key in ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps"):
        assert ref[key] == rev[key], key
    for key, val in got.items():
        const = pc.SPREAD[name][key]
        if key == "cost" and val < pc.cost_floor(sc):
            assert const <= 4.0 * pc.cost_floor(sc), (key, const)   # (bound() takes the floor anyway)
            continue
        assert val <= const <= 4.0 * val, (key, val, const)


@pytest.mark.parametrize("name", pc.SCENES)
def test_reference_ends_by_a_tolerance_test_far_from_every_threshold(name):
    ref = pc.reference(name)
    assert ref["ok"] == 1 and ref["termination"] in ("FUNCTION_TOLERANCE", "GRADIENT_TOLERANCE", "PARAMETER_TOLERANCE")
    assert ref["num_iterations"] <= 50 and ref["num_invalid_steps"] == 0
    for tq in ref["trace"][-2:]:
        for key, (val, thr) in tq.items():
            assert val > 2.0 * thr or val < 0.5 * thr, (name, key, val, thr)


def test_badloop12_turns_the_wrong_edge_off_and_ring8_reaches_zero():
    rho1 = pc.reference("badloop12")["rho1"]
    assert rho1[-1] < 0.05 and rho1[:-1].min() > 0.5, rho1
    assert pc.reference("ring8")["final_cost"] < 1e-20
    # the drift scene's log-scales are a ramp, not a constant
    sig = pc.reference("drift12")["x"][:, 7]
    assert sig[0] == 0.0 and np.ptp(sig[1:]) > 0.05


def test_two_comp_has_an_unanchored_component():
    sc = pc.scene("two_comp")
    assert sc["fixed"][:6].sum() == 1 and sc["fixed"][6:].sum() == 0
    assert not any((a < 6) != (b < 6) for a, b in sc["edges"])


def test_loop_closing_scene_orders_graph_before_one_rigid_similarity():
    r = pc.loop_reference()
    print("closing frames, rigid similarity: %.4g deg %.4g units; pose graph: %.4g deg %.4g units" %
          (*r["rigid"], *r["graph"]))
    assert r["ref"]["ok"] == 1 and r["ref"]["num_invalid_steps"] == 0
    assert 2.0 * r["graph"][0] <= r["rigid"][0] and 2.0 * r["graph"][1] <= r["rigid"][1]
