"""Cases, bounds and the comparison shared by the reduced-system shape tests of the bundle adjustment
(test_ba_shapes_reference_bounds.py on the CPU, test_ba_shapes_gpu.py on the device).

Every system has n = 6 (free frames).  A case (solve, r) is the sliding-window problem
    m = make_scene(num_frames=solve + 2, num_points=max(120, 40 (solve + 2)), seed=5, run_max=r)
    pa = ba.problem_from_map_frames(m, solve, solve + 2, 2.0)
solved with default_solver_options(max_num_iterations=3): n = 6 solve, NT = ceil(n / 16) tile rows of S, and the
run length r of a point's track sets the co-visibility band.  The comparator is always oracle.solve on a copy, with
the same options; on every case it takes 3 successful steps and none rejected or invalid, so the two trajectories
are compared iteration for iteration.

  size sweep   r = 14, solve = 1 .. 48: NT = 1 .. 18 (every value), every padding 16 NT - n in {0, 2, .., 14}
               (solve = 1 .. 8 already), one workgroup up to NT = 12 and the dissected band from kSplitMinNT = 13.
  band sweep   solve in {35, 46} (NT = 14, 18), r in {3, 4, 7, 10, 12, 16, 18, 19, 20, 26}: bands of 2 .. 8 tiles on
               k_chol_tiles with separators of 1 .. 7 tile rows, 9 and 11 tiles on k_cholesky_global.  (r = 2 is left
               out: points with two observations make the step ill-conditioned, and the oracle then differs from
               itself by 4.6e-9 in relative cost between 1 and 4 threads.)
  path sweep   the same problems with the kernel choice forced: SG_CHOL_WINDOW=1 (k_cholesky_window where the band
               fits its 128 columns, else k_cholesky_global with staged panel rows) and SG_CHOL_GSTAGE=0 on top of it
               (k_cholesky_global unstaged).  SG_CHOL_GSTAGE=0 alone at (9, 14) is not a case: with the window knob
               unset the planner keeps such a band on k_chol_tiles, so the knob selects nothing there.

The bounds are those of test_ba_gpu.py::test_c5_first_iterations_match_oracle.  The reference alone (1 thread
against 4 threads, and against its -ffast-math build) stays under half of each over all cases; measured: final cost
1.8e-11, q 1.4e-12, t 1.0e-7 mm, X 3.3e-11 (test_ba_shapes_reference_bounds.py recomputes them)."""
import numpy as np

from slamgpu import ba
from slamgpu.capi import default_solver_options
from slamgpu.scene import make_scene

ITERATIONS = 3
INITIAL_COST_REL = 1e-10
FINAL_COST_REL = 1e-9
Q_ABS = 1e-9
T_ABS_MM = 1e-6
X_ABS = 1e-9
COUNTERS = ("num_iterations", "num_successful_steps", "num_unsuccessful_steps")

SIZE_SWEEP = [(solve, 14) for solve in range(1, 49)]
BAND_RUNS = (3, 4, 7, 10, 12, 16, 18, 19, 20, 26)
BAND_SWEEP = [(solve, r) for solve in (35, 46) for r in BAND_RUNS]
BAND_SPLIT = [(solve, r) for solve, r in BAND_SWEEP if r <= 19]   # bands of at most 8 tiles: k_chol_tiles, dissected

PATH_WINDOW, PATH_STAGED, PATH_UNSTAGED = 1, 2, 3   # info()["cholesky_path"]
# (solve, r, knobs, info()["cholesky_path"])
PATH_SWEEP = (
    [(solve, 14, {"SG_CHOL_WINDOW": "1"}, PATH_WINDOW) for solve in (1, 2, 3, 9, 17, 21, 32, 35, 46)] +
    [(35, 3, {"SG_CHOL_WINDOW": "1"}, PATH_WINDOW), (35, 18, {"SG_CHOL_WINDOW": "1"}, PATH_WINDOW)] +
    [(solve, r, {"SG_CHOL_WINDOW": "1"}, PATH_STAGED) for solve, r in ((35, 20), (46, 26))] +
    [(solve, r, {"SG_CHOL_WINDOW": "1", "SG_CHOL_GSTAGE": "0"}, PATH_UNSTAGED) for solve, r in ((35, 20), (46, 26))])

_cache = {}


def options():
    return default_solver_options(max_num_iterations=ITERATIONS)


def tile_rows(n):
    return (n + 15) // 16


def problem(solve, r):
    """A fresh copy of case (solve, r)'s ProblemArrays."""
    key = ("problem", solve, r)
    if key not in _cache:
        frames = solve + 2
        m = make_scene(num_frames=frames, num_points=max(120, 40 * frames), seed=5, run_max=r)
        _cache[key] = ba.problem_from_map_frames(m, solve, frames, 2.0)
    return _cache[key].copy()


def oracle_result(oracle_lib, solve, r, nthreads=1, fastmath=False):
    """(summary, solved ProblemArrays) of oracle.solve on case (solve, r): computed once, left unchanged."""
    key = ("oracle", solve, r, nthreads, fastmath)
    if key not in _cache:
        pa = problem(solve, r)
        s = oracle_lib.solve(pa, options(), nthreads=nthreads, fastmath=fastmath)
        _cache[key] = (s, pa)
    return _cache[key]


def _rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a - b)


ROWS = ("initial cost rel", "final cost rel", "q", "t mm", "X")
_sweep_worst = {}


def compare(label, sweep, results, share=1.0):
    """results: [(case name, summary, ProblemArrays, reference summary, reference ProblemArrays)].  Prints the worst
    value of each row, over these cases and over everything compared so far under the name sweep, then asserts the
    counters and the bounds (share = 0.5: half of each, the reference against itself)."""
    worst = {row: (0.0, "-") for row in ROWS}
    wrong = []
    for name, s, p, rs, rp in results:
        if not (s["ok"] == rs["ok"] == 1) or any(s[k] != rs[k] for k in COUNTERS) or \
                rs["num_successful_steps"] != ITERATIONS or rs["num_unsuccessful_steps"] != 0:
            wrong.append((name, {k: (s[k], rs[k]) for k in COUNTERS + ("ok",)}))
        figures = (_rel(s["initial_cost"], rs["initial_cost"]), _rel(s["final_cost"], rs["final_cost"]),
                   np.abs(p.q - rp.q).max(), np.abs(p.t - rp.t).max(), np.abs(p.X - rp.X).max())
        for row, v in zip(ROWS, figures):
            v = float(v) if np.isfinite(v) else float("inf")
            if v >= worst[row][0]:
                worst[row] = (v, name)
    total = _sweep_worst.setdefault(sweep, {row: (0.0, "-") for row in ROWS})
    for row in ROWS:
        if worst[row][0] >= total[row][0]:
            total[row] = worst[row]
    print("%s, %d cases, %d iterations: %s" % (label, len(results), ITERATIONS, "; ".join(
        "%s %.2e (%s)" % (row, worst[row][0], worst[row][1]) for row in ROWS)))
    print("  %s so far: %s" % (sweep, "; ".join("%s %.2e (%s)" % (row, total[row][0], total[row][1]) for row in ROWS)))
    assert not wrong, wrong
    for row, bound in zip(ROWS, (INITIAL_COST_REL, FINAL_COST_REL, Q_ABS, T_ABS_MM, X_ABS)):
        assert worst[row][0] <= share * bound, (row, worst[row], share * bound)
