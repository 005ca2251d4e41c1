"""Inputs, the per-point oracle problem and the comparison bounds shared by the structure-only bundle adjustment
tests (test_points_reference_bounds.py on the CPU, test_points_gpu.py on the device).

The comparator is always oracle.solve on the problem built here from the MapArrays: the point's enabled
observations in map order, those observations' frames constant (frame_rot_free = frame_trans_free = 0), the one
point free, no distance blocks, range 2.0.

The problem is ill-conditioned in depth and stops on function_tolerance, so a rounding-level change moves a
minority of points to another iteration count.  The bounds below are 3-5x the spread of the reference against
itself (the strict oracle against its -ffast-math build, on scenes A and B and two smaller ones at seeds 1 and 2);
test_points_reference_bounds.py recomputes that spread."""
import numpy as np

from slamgpu.capi import ProblemArrays, default_solver_options
from slamgpu.scene import make_config, make_scene

RANGE = 2.0
COUNTERS = ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps", "termination",
            "ok")

# first 5 LM iterations (max_num_iterations = 5)
IT5_DIFFERENT_POINTS = 0      # points whose counters, termination or ok differ
IT5_COST_REL = 1e-10          # final cost, relative (reference alone: 2.6e-11)
IT5_X_REL = 1e-10             # max |dX| / max |X| (reference alone: 1.5e-11)
# converged (default options)
CONV_OK_DIFFERENT_POINTS = 0  # points whose ok differs
CONV_DIFFERENT_SHARE = 0.20   # share of points whose counters or termination differ (reference alone: 11 %)
CONV_SAME_COST_REL = 1e-6     # counters equal: final cost, relative (reference alone: 1.8e-7)
CONV_SAME_RES_PX = 5e-3       # counters equal: residuals through oracle.evaluate (reference alone: 1.4e-3 px)
CONV_ANY_COST_REL = 2e-5      # every point with ok = 1 (reference alone: 6.0e-6)
CONV_ANY_RES_PX = 0.1         # every point with ok = 1 (reference alone: 2.8e-2 px)
INITIAL_COST_REL = 1e-10

_cache = {}


def scene(name):
    """A: make_config("C1"), 10 frames, 484 points, 2-10 observations each.  B: make_scene(40, 400, 7,
    run_max=40), 40 frames, 391 points, 2-37 observations each (7, 8, 9, 16, 17 and 33 all occur)."""
    if name not in _cache:
        _cache[name] = make_config("C1") if name == "A" else make_scene(40, 400, 7, run_max=40)
    return _cache[name].copy()


def start(m, seed):
    """Every point's depth off by -40 .. +60 % and a small tilt."""
    rng = np.random.default_rng(seed)
    P = m.num_points
    X = m.X.reshape(-1, 4)
    X[:, 3] *= rng.uniform(0.6, 1.6, P)
    X[:, :3] += rng.normal(0, 2e-3, (P, 3))
    return m


def started(name, seed=1):
    return start(scene(name), seed)


def enabled_obs(m, p):
    return np.flatnonzero((m.obs_point == p) & (m.obs_disabled == 0))


def point_problem(m, p, X=None):
    """The Ceres problem in which only point p is free, as ProblemArrays (X: another location for p)."""
    sel = enabled_obs(m, p)
    fr, inv = np.unique(m.obs_frame[sel], return_inverse=True)
    z = np.zeros(len(fr), dtype=np.uint8)
    return ProblemArrays(
        k=m.k.copy(), q=m.q.reshape(-1, 4)[fr].copy(), t=m.t.reshape(-1, 3)[fr].copy(),
        frame_camera=m.frame_camera[fr], frame_rot_free=z, frame_trans_free=z,
        X=(m.X[4 * p:4 * p + 4] if X is None else np.asarray(X)).copy(), point_free=[1],
        obs_pt=m.obs_pt.reshape(-1, 2)[sel].copy(), obs_frame=inv, obs_point=np.zeros(len(sel), dtype=np.int32),
        dist_frame=[], dist_prev=[], range_=RANGE, frame_map_index=fr, point_map_index=[p])


def oracle_points(oracle_lib, m, points, options=None, fastmath=False):
    """oracle.solve on each listed point's problem: (summaries, X[len(points)][4]).  A point whose solve ends with
    ok = 0 keeps its X, as the call under test leaves it."""
    sums, X = [], np.zeros((len(points), 4))
    for i, p in enumerate(points):
        pa = point_problem(m, p)
        s = oracle_lib.solve(pa, options or default_solver_options(), fastmath=fastmath)
        sums.append(s)
        X[i] = pa.X if s["ok"] else m.X[4 * p:4 * p + 4]
    return sums, X


def cached_oracle(oracle_lib, name, iters, fastmath=False):
    """The oracle on every point of started(name, 1), computed once and left unchanged."""
    key = ("oracle", name, iters, fastmath)
    if key not in _cache:
        m = started(name)
        o = default_solver_options(max_num_iterations=iters) if iters else default_solver_options()
        _cache[key] = oracle_points(oracle_lib, m, list(range(m.num_points)), o, fastmath)
    sums, X = _cache[key]
    return [dict(s) for s in sums], X.copy()


def residuals(oracle_lib, m, p, X):
    """Residuals (px) of point p at X through oracle.evaluate; None if it projects behind a camera."""
    r, _, nf = oracle_lib.evaluate(point_problem(m, p, X))
    return r if nf == 0 else None


def same_counters(a, b):
    return all(a[k] == b[k] for k in COUNTERS)


def _rel(a, b):
    return abs(a - b) / b if b else abs(a - b)


def compare_it5(label, m, points, sums, X, ref_sums, ref_X):
    """The 5-iteration rows: prints the worst value of each, then asserts the bounds."""
    different = [p for i, p in enumerate(points) if not same_counters(sums[i], ref_sums[i])]
    ran = [i for i in range(len(points)) if ref_sums[i]["ok"]]
    cost = max(_rel(sums[i]["final_cost"], ref_sums[i]["final_cost"]) for i in ran)
    init = max(_rel(sums[i]["initial_cost"], ref_sums[i]["initial_cost"]) for i in range(len(points)))
    dx = np.abs(X[ran] - ref_X[ran]).max() / np.abs(ref_X[ran]).max()
    print("%s, 5 iterations, %d points: %d differ in counters %s; final cost %.2e rel; X %.2e rel; initial cost "
          "%.2e rel" % (label, len(points), len(different), different[:8], cost, dx, init))
    assert len(different) <= IT5_DIFFERENT_POINTS
    assert cost <= IT5_COST_REL
    assert dx <= IT5_X_REL
    assert init <= INITIAL_COST_REL


def compare_converged(label, oracle_lib, m, points, sums, X, ref_sums, ref_X):
    """The converged rows.  m: the map the points were solved against (their frames and observations)."""
    n = len(points)
    ok_differs = [p for i, p in enumerate(points) if sums[i]["ok"] != ref_sums[i]["ok"]]
    different = [i for i in range(n) if not same_counters(sums[i], ref_sums[i])]
    worst = {"same": [0.0, 0.0], "any": [0.0, 0.0]}
    behind = []
    for i, p in enumerate(points):
        if not (sums[i]["ok"] and ref_sums[i]["ok"]):
            continue
        cost = _rel(sums[i]["final_cost"], ref_sums[i]["final_cost"])
        r, rr = residuals(oracle_lib, m, p, X[i]), residuals(oracle_lib, m, p, ref_X[i])
        if r is None or rr is None:
            behind.append(p)
            continue
        res = np.abs(r - rr).max()
        for row in (("any",) if i in different else ("same", "any")):
            worst[row] = [max(worst[row][0], cost), max(worst[row][1], res)]
    init = max(_rel(sums[i]["initial_cost"], ref_sums[i]["initial_cost"]) for i in range(n))
    print("%s, converged, %d points: ok differs on %s; %d (%.1f %%) differ in counters; counters equal: cost %.2e "
          "rel, residuals %.2e px; every ok point: cost %.2e rel, residuals %.2e px; initial cost %.2e rel" % (
              label, n, ok_differs, len(different), 100.0 * len(different) / n, worst["same"][0], worst["same"][1],
              worst["any"][0], worst["any"][1], init))
    assert len(ok_differs) <= CONV_OK_DIFFERENT_POINTS
    assert not behind, behind
    assert len(different) <= CONV_DIFFERENT_SHARE * n
    assert worst["same"][0] <= CONV_SAME_COST_REL and worst["same"][1] <= CONV_SAME_RES_PX
    assert worst["any"][0] <= CONV_ANY_COST_REL and worst["any"][1] <= CONV_ANY_RES_PX
    assert init <= INITIAL_COST_REL
