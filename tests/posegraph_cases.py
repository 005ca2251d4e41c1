"""Shared inputs and the numpy reference of the pose-graph tests (sg_slam_optimize_pose_graph, sg_map_pose_edges,
sg_map_covisible_pairs).

The reference is restated here in numpy from the formulas of include/slamgpu.h and is never another path of the
library.  It is dense: the residual of every edge, an analytic Jacobian written with the 4x4 left / right product
matrices and the closed derivative of R(q) d (not the cross-product form of csrc/posegraph_math.h), checked against
central differences by tests/test_posegraph_reference_bounds.py, and the Ceres 1.8 Levenberg-Marquardt loop
(TrustRegionMinimizer + LevenbergMarquardtStrategy: Jacobi scaling from iteration 0, the clamped diagonal, the model
cost change from J, the step decision) with numpy.linalg.cholesky on the full matrix.

A scene is a dict: q (N, 4) and t (N, 3) the poses at entry, fixed (N), edges (E, 2), meas (E, 8), weights (E, 3),
range, fix_scale, and where there is one q_true, t_true.  Quaternions are Eigen memory [x, y, z, w], the map's
p = R(q)(X - t)."""
import numpy as np

from slamgpu.scene import MapArrays, axis_angle, quat_from_matrix, quat_to_matrix

MARGIN = 100.0
EPS = 2.0 ** -52
W_ROT, W_T, W_S = 1000.0, 1.0, 300.0   # per radian, per map unit, per unit of log-scale
BAD_RANGE = 30.0                        # CauchyLoss range of badloop12

OPTIONS = dict(max_num_iterations=1000, function_tolerance=1e-7, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
               min_relative_decrease=1e-3, initial_trust_region_radius=1e4, max_trust_region_radius=1e16,
               min_trust_region_radius=1e-32, min_lm_diagonal=1e-6, max_lm_diagonal=1e32,
               max_num_consecutive_invalid_steps=5, jacobi_scaling=1)

# Solver options per scene where Ceres' defaults would end the exact ring three orders of magnitude above the cost's
# rounding floor: ring8 runs until the step itself vanishes.
SCENE_OPTIONS = {"ring8": dict(parameter_tolerance=1e-12, gradient_tolerance=1e-18)}

SCENES = ("ring8", "drift12", "chords24", "rigid12", "badloop12", "long300",
          "far12", "farrigid12", "farcauchy12", "complete48", "star40")

# Scenes that do not end converged, each with the options that take it there.  They stay out of SCENES: their result
# is a status, a termination type and the four step counts (and for maxiter the states after two steps), not a minimum.
#   loose9, loose9_3   ring8's ring and a node 8 that hangs on one edge (3, 8) of weight LOOSE_W; with min_lm_diagonal = 0
#                      the node's damped block is exactly 0, every step meets a pivot that is exactly 0 (invalid) and the
#                      solve ends NUMERICAL_FAILURE after max_num_consecutive_invalid_steps of them (5, and 3).  The
#                      planner's ties go to the lower list position, so node 8 is the last column, a column without rows;
#   loose_first9       the same with the loose node at list position 1 (on the edge (4, 1)): the first column;
#   loose_last9        the loose node joined to every ring node: the last column, below a block in every other column;
#   maxiter_chords24   chords24 stopped by max_num_iterations = 2: NO_CONVERGENCE;
#   minradius_far12    far12 with min_trust_region_radius = 2000: the first steps are rejected and the radius test ends it.
PATH_SCENES = ("loose9", "loose9_3", "loose_first9", "loose_last9", "maxiter_chords24", "minradius_far12")
LOOSE_NODE = {"loose9": 8, "loose9_3": 8, "loose_first9": 1, "loose_last9": 8}
LOOSE_W = 1e-200                        # J is of order 1e-197: J^T J and J^T r underflow to exactly 0
SCENE_OPTIONS.update({
    "loose9": dict(min_lm_diagonal=0.0),
    "loose9_3": dict(min_lm_diagonal=0.0, max_num_consecutive_invalid_steps=3),
    "loose_first9": dict(min_lm_diagonal=0.0),
    "loose_last9": dict(min_lm_diagonal=0.0),
    "maxiter_chords24": dict(max_num_iterations=2),
    "minradius_far12": dict(min_trust_region_radius=2000.0),
})

# The reference's own rounding floor per scene: the worst difference between the reference solved with the nodes and
# edges in listed order and in reversed order, in rotation (deg), centre (map units), log-scale and final cost.
# tests/test_posegraph_reference_bounds.py recomputes them and fails when a value is not an upper bound within a factor
# of 4.  The code under test gets MARGIN times them: another elimination order, a sparse factor, another summation
# order and FMA contraction.  The cost's entry is never taken below cost_floor(scene).
SPREAD = {
    "ring8": {"rot_deg": 1.8e-14, "t": 8.2e-13, "log_scale": 4.5e-16, "cost": 1.6e-25},
    "drift12": {"rot_deg": 3.8e-14, "t": 6.1e-13, "log_scale": 4.5e-16, "cost": 2.8e-12},
    "chords24": {"rot_deg": 4e-14, "t": 4.1e-13, "log_scale": 7.1e-16, "cost": 1.5e-19},
    "rigid12": {"rot_deg": 3.7e-14, "t": 4.1e-13, "log_scale": 0.0, "cost": 1.4e-12},
    "badloop12": {"rot_deg": 3.6e-14, "t": 6.1e-13, "log_scale": 3.5e-16, "cost": 8.2e-12},
    "long300": {"rot_deg": 3.9e-14, "t": 2.5e-12, "log_scale": 4.3e-16, "cost": 5.7e-18},
    "far12": {"rot_deg": 5.6e-14, "t": 1.6e-12, "log_scale": 7.6e-16, "cost": 2.1e-16},
    "farrigid12": {"rot_deg": 6.9e-14, "t": 1.6e-12, "log_scale": 0.0, "cost": 2.8e-18},
    "farcauchy12": {"rot_deg": 2.5e-14, "t": 1.1e-12, "log_scale": 2.3e-15, "cost": 0.0},
    "complete48": {"rot_deg": 2.4e-14, "t": 4.5e-13, "log_scale": 1.8e-15, "cost": 2.8e-14},
    "star40": {"rot_deg": 3.7e-14, "t": 6.8e-13, "log_scale": 1.4e-19, "cost": 1.0e-18},
    "maxiter_chords24": {"rot_deg": 2.9e-14, "t": 4.5e-13, "log_scale": 6.6e-16, "cost": 4.6e-16},
}

_cache = {}


# ---------------------------------------------------------------------------------------------- quaternions
def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def qconj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


def qunit(q):
    q = np.asarray(q, float) / np.linalg.norm(q)
    return -q if q[3] < 0 else q


def left_matrix(p):
    """p (x) q = left_matrix(p) @ q."""
    x, y, z, w = p
    return np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]])


def right_matrix(p):
    """q (x) p = right_matrix(p) @ q."""
    x, y, z, w = p
    return np.array([[w, z, -y, x], [-z, w, x, y], [y, -x, w, z], [-x, -y, -z, w]])


def quat_plus(x, d):
    """ceres::QuaternionParameterization::Plus applied to Eigen memory (csrc/project_math.h, QuatPlus)."""
    nd = np.linalg.norm(d)
    if nd == 0.0:
        return np.array(x, float)
    s = np.sin(nd) / nd
    z0, z1, z2, z3 = np.cos(nd), s * d[0], s * d[1], s * d[2]
    return np.array([z0 * x[0] - z1 * x[1] - z2 * x[2] - z3 * x[3], z0 * x[1] + z1 * x[0] + z2 * x[3] - z3 * x[2],
                     z0 * x[2] - z1 * x[3] + z2 * x[0] + z3 * x[1], z0 * x[3] + z1 * x[2] - z2 * x[1] + z3 * x[0]])


def quat_local(x):
    """Its Jacobian at 0 (4 x 3)."""
    return np.array([[-x[1], -x[2], -x[3]], [x[0], x[3], -x[2]], [-x[3], x[0], x[1]], [x[2], -x[1], x[0]]])


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def rot_err_deg(qa, qb):
    e = qmul(qa, qconj(qb))
    return float(np.degrees(2.0 * np.arctan2(np.linalg.norm(e[:3]), abs(e[3]))))


# ---------------------------------------------------------------------------------------------- the residual
def edge_residual(xa, xb, meas, w, fix_scale):
    """r (7) of one edge at the states xa, xb (q 4 | t 3 | sigma), before the loss."""
    e = qmul(qmul(qconj(meas[:4]), xa[:4]), qconj(xb[:4]))
    if e[3] < 0:
        e = -e
    th = np.linalg.norm(e[:3])
    om = (2.0 * np.arctan2(th, e[3]) / th) * e[:3] if th > 1e-150 else 2.0 * e[:3] / e[3]
    es = 1.0 if fix_scale else np.exp(-xa[7])
    rt = es * quat_to_matrix(xa[:4]) @ (xb[4:7] - xa[4:7]) - meas[4:7]
    rs = 0.0 if fix_scale else w[2] * (xb[7] - xa[7] - meas[7])
    return np.concatenate([w[0] * om, w[1] * rt, [rs]])


def edge_jacobian(xa, xb, meas, w, fix_scale):
    """The analytic 7 x 14 Jacobian of edge_residual in the local coordinates (rot 3 | t 3 | sigma per node)."""
    c, d = qconj(meas[:4]), qconj(xb[:4])
    m = qmul(c, xa[:4])
    e = qmul(m, d)
    s = -1.0 if e[3] < 0 else 1.0
    e = s * e
    v, ww = e[:3], e[3]
    th2 = v @ v
    n2 = th2 + ww * ww
    if th2 < 1e-12:
        g, h = 2.0 / ww, -4.0 / (3.0 * ww ** 3)
    else:
        th = np.sqrt(th2)
        g = 2.0 * np.arctan2(th, ww) / th
        h = (2.0 * ww / n2 - g) / th2
    dlog = np.concatenate([g * np.eye(3) + h * np.outer(v, v), (-2.0 / n2 * v)[:, None]], 1)   # 3 x 4
    J = np.zeros((7, 14))
    J[0:3, 0:3] = w[0] * s * dlog @ left_matrix(c) @ right_matrix(d) @ quat_local(xa[:4])
    J[0:3, 7:10] = w[0] * s * dlog @ left_matrix(m) @ np.diag([-1.0, -1.0, -1.0, 1.0]) @ quat_local(xb[:4])
    qv, qw = xa[:3], xa[3]
    dd = xb[4:7] - xa[4:7]
    # R(q) d = d + 2 w (v x d) + 2 (v (v.d) - d (v.v))
    dRd = np.concatenate([-2.0 * qw * skew(dd) + 2.0 * ((qv @ dd) * np.eye(3) + np.outer(qv, dd) - 2.0 * np.outer(dd, qv)),
                          (2.0 * np.cross(qv, dd))[:, None]], 1)   # 3 x 4
    es = 1.0 if fix_scale else np.exp(-xa[7])
    R = quat_to_matrix(xa[:4])
    J[3:6, 0:3] = w[1] * es * dRd @ quat_local(xa[:4])
    J[3:6, 3:6] = -w[1] * es * R
    J[3:6, 10:13] = w[1] * es * R
    if not fix_scale:
        J[3:6, 6] = -w[1] * es * (R @ dd)
        J[6, 6], J[6, 13] = -w[2], w[2]
    return J


def node_plus(x, d, fix_scale):
    out = np.array(x, float)
    out[:4] = quat_plus(x[:4], d[:3])
    out[4:7] = x[4:7] + d[3:6]
    if not fix_scale:
        out[7] = x[7] + d[6]
    return out


# ---------------------------------------------------------------------------------------------- the reference LM
def evaluate(sc, x, jac=True):
    """Corrected residuals (E, 7), corrected Jacobians (E, 7, 14) or None, the cost over the edges with a free node,
    the fixed cost and rho' per edge."""
    E = len(sc["edges"])
    fs, b = sc["fix_scale"], sc["range"] ** 2
    r = np.zeros((E, 7))
    J = np.zeros((E, 7, 14)) if jac else None
    rho1 = np.ones(E)
    cost = fixed = 0.0
    for i, (a, bb) in enumerate(sc["edges"]):
        ri = edge_residual(x[a], x[bb], sc["meas"][i], sc["weights"][i], fs)
        s2 = float(ri @ ri)
        c = 0.5 * s2
        if b > 0:
            rho1[i] = 1.0 / (1.0 + s2 / b)
            c = 0.5 * b * np.log(1.0 + s2 / b)
        sr = np.sqrt(rho1[i])
        r[i] = sr * ri
        if sc["fixed"][a] and sc["fixed"][bb]:
            fixed += c
            continue
        cost += c
        if jac:
            J[i] = sr * edge_jacobian(x[a], x[bb], sc["meas"][i], sc["weights"][i], fs)
    return r, J, cost, fixed, rho1


def solve_np(sc, options=None):
    """The Ceres 1.8 LM on the scene, dense.  Returns a dict: x (N, 8), the summary fields, rho1 per edge at the
    result and `trace`, per iteration the termination quantities as (value, threshold) pairs, and under "decision" the
    step's relative decrease with min_relative_decrease."""
    o = dict(OPTIONS)
    o.update(options or {})
    fs = sc["fix_scale"]
    D = 6 if fs else 7
    N = len(sc["q"])
    free = [i for i in range(N) if not sc["fixed"][i]]
    col = {nd: j for j, nd in enumerate(free)}
    n = D * len(free)
    x = np.zeros((N, 8))
    x[:, :4], x[:, 4:7] = sc["q"], sc["t"]

    def dense(r, J):
        A = np.zeros((7 * len(sc["edges"]), n))
        for i, (a, b) in enumerate(sc["edges"]):
            if a in col:
                A[7 * i:7 * i + 7, D * col[a]:D * col[a] + D] = J[i][:, 0:D]
            if b in col:
                A[7 * i:7 * i + 7, D * col[b]:D * col[b] + D] = J[i][:, 7:7 + D]
        return A, r.reshape(-1)

    def xnorm(xx):
        return float(np.sqrt(sum((xx[i, :7 if fs else 8] ** 2).sum() for i in free)))

    r, J, cost, fixed, rho1 = evaluate(sc, x)
    A, rv = dense(r, J)
    g = A.T @ rv
    gmax = float(np.abs(g).max())
    scale = 1.0 / (1.0 + np.sqrt((A * A).sum(0))) if o["jacobi_scaling"] else np.ones(n)
    abs_gtol = o["gradient_tolerance"] * gmax
    res = dict(initial_cost=cost + fixed, fixed_cost=fixed, num_iterations=1, num_successful_steps=0,
               num_unsuccessful_steps=0, num_invalid_steps=0, termination="NO_CONVERGENCE", ok=1)
    min_cost, x_norm = cost, xnorm(x)
    radius, dec, reuse, diag = o["initial_trust_region_radius"], 2.0, False, None
    trace, consecutive_invalid, done = [], 0, gmax <= abs_gtol
    if done:
        res["termination"] = "GRADIENT_TOLERANCE"
    while not done:
        if res["num_iterations"] - 1 >= o["max_num_iterations"]:
            break
        As = A * scale
        if not reuse:
            diag = np.clip((As * As).sum(0), o["min_lm_diagonal"], o["max_lm_diagonal"])
        H = As.T @ As + np.diag(diag / radius)
        tq = {"gradient": (gmax, abs_gtol), "radius": (radius, o["min_trust_region_radius"])}
        trace.append(tq)
        valid = True
        try:
            L = np.linalg.cholesky(H)
            y = np.linalg.solve(L.T, np.linalg.solve(L, As.T @ rv))
        except np.linalg.LinAlgError:
            valid = False
        if valid:
            delta = -y * scale
            jd = A @ delta
            model = -float(jd @ (rv + 0.5 * jd))
            valid = np.isfinite(model) and not model < 0.0
        if not valid:
            res["num_invalid_steps"] += 1
            consecutive_invalid += 1
            if consecutive_invalid >= o["max_num_consecutive_invalid_steps"]:
                res["termination"], res["ok"] = "NUMERICAL_FAILURE", 0
                break
            accepted = False
        else:
            consecutive_invalid = 0
            xc = x.copy()
            for nd in free:
                xc[nd] = node_plus(x[nd], delta[D * col[nd]:D * col[nd] + D], fs)
            step_norm = float(np.sqrt(sum(((xc[i] - x[i])[:7 if fs else 8] ** 2).sum() for i in free)))
            tq["parameter"] = (step_norm, o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]))
            if step_norm <= tq["parameter"][1]:
                res["termination"] = "PARAMETER_TOLERANCE"
                break
            rc, Jc, new_cost, _, rho1c = evaluate(sc, xc)
            change = cost - new_cost
            tq["function"] = (abs(change), o["function_tolerance"] * cost)
            if abs(change) < tq["function"][1]:
                res["termination"] = "FUNCTION_TOLERANCE"
                break
            rel = change / model
            tq["decision"] = (rel, o["min_relative_decrease"])
            accepted = rel > o["min_relative_decrease"]
        if accepted:
            res["num_successful_steps"] += 1
            radius = min(o["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
            dec, reuse = 2.0, False
            x, r, J, cost, rho1 = xc, rc, Jc, new_cost, rho1c
            x_norm = xnorm(x)
            A, rv = dense(r, J)
            g = A.T @ rv
            gmax = float(np.abs(g).max())
            if gmax <= abs_gtol or radius < o["min_trust_region_radius"]:
                res["termination"] = "GRADIENT_TOLERANCE" if gmax <= abs_gtol else "PARAMETER_TOLERANCE"
                trace.append({"gradient": (gmax, abs_gtol), "radius": (radius, o["min_trust_region_radius"])})
                break
        else:
            res["num_unsuccessful_steps"] += 1
            radius /= dec
            dec *= 2.0
            reuse = True
            if radius < o["min_trust_region_radius"]:
                res["termination"] = "PARAMETER_TOLERANCE"
                break
        res["num_iterations"] += 1
        min_cost = min(min_cost, cost)
    res.update(x=x, final_cost=min_cost + fixed, rho1=rho1, trace=trace)
    return res


def reversed_scene(sc):
    """The same problem with the nodes and the edges listed backwards."""
    N = len(sc["q"])
    out = dict(sc)
    for k in ("q", "t", "fixed", "q_true", "t_true"):
        if sc.get(k) is not None:
            out[k] = sc[k][::-1].copy()
    out["edges"] = (N - 1 - sc["edges"])[::-1].copy()
    out["meas"], out["weights"] = sc["meas"][::-1].copy(), sc["weights"][::-1].copy()
    return out


def compare(xa, xb):
    """Worst differences between two (N, 8) state arrays: rotation deg, centre, log-scale."""
    return {"rot_deg": max(rot_err_deg(qunit(a[:4]), qunit(b[:4])) for a, b in zip(xa, xb)),
            "t": float(np.abs(xa[:, 4:7] - xb[:, 4:7]).max()), "log_scale": float(np.abs(xa[:, 7] - xb[:, 7]).max())}


def cost_floor(sc):
    """What fp64 leaves of a final cost near zero: every residual component comes from terms of size w_t |t| with a
    few roundings each, so the cost is not known below 0.5 * 7 E (4 eps M)^2."""
    M = float(np.max(sc["weights"][:, 1]) * np.abs(sc["t"]).max())
    return 0.5 * 7 * len(sc["edges"]) * (4.0 * EPS * M) ** 2


def bound(name, key):
    v = SPREAD[name][key]
    if key == "cost":
        v = max(v, cost_floor(scene(name)))
    return MARGIN * v


def reference(name):
    if ("ref", name) not in _cache:
        _cache[("ref", name)] = solve_np(scene(name), SCENE_OPTIONS.get(name))
    return _cache[("ref", name)]


def reversed_reference(name):
    """The reference on the scene listed backwards (its x is in reversed node order)."""
    if ("rev", name) not in _cache:
        _cache[("rev", name)] = solve_np(reversed_scene(scene(name)), SCENE_OPTIONS.get(name))
    return _cache[("rev", name)]


def entry_matrix(sc, options=None):
    """The first step's dense matrix S J^T J S + D / radius at the entry state, as solve_np builds it, and the free
    nodes in its block order."""
    o = dict(OPTIONS)
    o.update(options or {})
    D = 6 if sc["fix_scale"] else 7
    free = [i for i in range(len(sc["q"])) if not sc["fixed"][i]]
    col = {nd: j for j, nd in enumerate(free)}
    x = np.zeros((len(sc["q"]), 8))
    x[:, :4], x[:, 4:7] = sc["q"], sc["t"]
    _, J, _, _, _ = evaluate(sc, x)
    A = np.zeros((7 * len(sc["edges"]), D * len(free)))
    for i, (a, b) in enumerate(sc["edges"]):
        if a in col:
            A[7 * i:7 * i + 7, D * col[a]:D * col[a] + D] = J[i][:, 0:D]
        if b in col:
            A[7 * i:7 * i + 7, D * col[b]:D * col[b] + D] = J[i][:, 7:7 + D]
    As = A * (1.0 / (1.0 + np.sqrt((A * A).sum(0))) if o["jacobi_scaling"] else 1.0)
    diag = np.clip((As * As).sum(0), o["min_lm_diagonal"], o["max_lm_diagonal"])
    return As.T @ As + np.diag(diag / o["initial_trust_region_radius"]), free


def column_rows(sc):
    """The planner's elimination order restated (csrc/posegraph_plan.cpp: greedy minimum degree on the block graph of
    the free nodes with an exact fill simulation, ties to the lower list position): per column in elimination order
    (node, number of off-diagonal blocks of L below its diagonal block)."""
    free = [i for i in range(len(sc["q"])) if not sc["fixed"][i]]
    adj = {i: set() for i in free}
    for a, b in sc["edges"]:
        if a in adj and b in adj:
            adj[int(a)].add(int(b))
            adj[int(b)].add(int(a))
    out = []
    while adj:
        v = min(adj, key=lambda i: (len(adj[i]), i))
        nb = adj.pop(v)
        out.append((v, len(nb)))
        for p in nb:
            adj[p].discard(v)
            adj[p] |= nb - {p}
    return out


def compute_cap1024():
    """cap1024 by the reference, listed and reversed: what tests/golden/posegraph_cap1024.npz holds.  Dense, 7161
    unknowns: minutes, and about 6 GB."""
    sc = scene("cap1024")
    ref = solve_np(sc)
    rev = solve_np(reversed_scene(sc))
    spread = compare(ref["x"], rev["x"][::-1])
    spread["cost"] = abs(ref["final_cost"] - rev["final_cost"])
    out = {k: ref[k] for k in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps",
                               "ok", "termination", "initial_cost", "final_cost", "x", "trace")}
    out.update(x_reversed=rev["x"][::-1].copy(), spread=spread,
               reversed_counts={k: rev[k] for k in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps",
                                                    "num_invalid_steps", "ok", "termination")})
    return out


def golden_cap1024():
    """The committed reference result of cap1024 (tests/golden/make_posegraph_golden.py; the dense solve takes
    minutes): x and x_reversed (N, 8, the latter in listed node order), the summary fields and `spread`, the listed
    against reversed differences."""
    if "golden_cap1024" not in _cache:
        import os
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posegraph_cap1024.npz")) as z:
            g = {k: z[k] for k in z.files}
        out = {k: int(g[k]) for k in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps",
                                      "num_invalid_steps", "ok")}
        out.update(x=g["x"], x_reversed=g["x_reversed"], termination=str(g["termination"]),
                   initial_cost=float(g["initial_cost"]), final_cost=float(g["final_cost"]),
                   spread={k: float(g["spread_" + k]) for k in ("rot_deg", "t", "log_scale", "cost")})
        _cache["golden_cap1024"] = out
    return _cache["golden_cap1024"]


def solver_options(name):
    """The scene's sg_solver_options (slamgpu.capi.SgSolverOptions)."""
    from slamgpu.capi import default_solver_options
    return default_solver_options(**SCENE_OPTIONS.get(name, {}))


def states(m, frames, log_scale):
    """(N, 8) states of the listed frames of a map, with the returned log-scales."""
    x = np.zeros((len(frames), 8))
    x[:, :4] = m.q.reshape(-1, 4)[frames]
    x[:, 4:7] = m.t.reshape(-1, 3)[frames]
    x[:, 7] = log_scale
    return x


def check_cap1024(x, out):
    """cap1024's result (x (1024, 8) states, out the graph's result) against the committed reference result: counts and
    termination equal, states within MARGIN times the golden's own listed-against-reversed spread, the final cost
    within MARGIN * max(that spread, cost_floor), and the error against the truth by ring8's rule."""
    g, sc = golden_cap1024(), scene("cap1024")
    keys = ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps")
    print("cap1024", {k: out[k] for k in ("status", "termination") + keys + ("final_cost",)},
          "the reference:", {k: g[k] for k in ("termination",) + keys + ("final_cost",)})
    assert out["status"] == "OK" and out["ok"] == 1 and out["termination"] == g["termination"]
    for key in keys:
        assert out[key] == g[key], (key, out[key], g[key])
    assert abs(out["initial_cost"] - g["initial_cost"]) <= 1e-12 * g["initial_cost"]
    d = compare(x, g["x"])
    d["cost"] = abs(out["final_cost"] - g["final_cost"])
    bounds = {k: MARGIN * g["spread"][k] for k in d}
    bounds["cost"] = MARGIN * max(g["spread"]["cost"], cost_floor(sc))
    print("cap1024 against the reference:", d, "bounds:", bounds)
    for key, val in d.items():
        assert val <= bounds[key], (key, val, bounds[key])
    xt = np.zeros_like(x)
    xt[:, :4], xt[:, 4:7] = sc["q_true"], sc["t_true"]
    own, got = compare(g["x"], xt), compare(x, xt)
    print("cap1024 against the truth:", got, "the reference:", own)
    for key in got:
        assert got[key] <= MARGIN * max(own[key], g["spread"][key]), key
    assert (x[0, :4] == sc["q"][0]).all() and (x[0, 4:7] == sc["t"][0]).all() and x[0, 7] == 0.0
    assert (np.abs(np.linalg.norm(x[1:, :4], axis=1) - 1.0) <= 4e-16).all() and (x[1:, 3] >= 0).all()


def written_back_q(q, fixed):
    """What the write-back of an SG_PG_OK graph leaves of the quaternions q (N, 4) when no step was accepted
    (include/slamgpu.h: "q_f normalised with w >= 0 ... of its free nodes"; csrc/posegraph_plan.cpp, PgWriteBack): the
    normalisation moves a unit quaternion by an ulp here and there, and it is applied whether or not the node moved."""
    q = np.array(q, float)
    rn = 1.0 / np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + (q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]))
    rn = np.where(q[:, 3] < 0.0, -rn, rn)
    return np.where(np.asarray(fixed, bool)[:, None], q, q * rn[:, None])


def check_path_result(name, out, m, before):
    """What the CPU executor and the device are both held to on a scene of PATH_SCENES solved alone on a map of its
    frames: `out` the graph's result, `m` the map after the call, `before` a copy from before it.

    A FAILED graph's frames are untouched bit for bit.  minradius_far12 ends OK without an accepted step, and an OK
    graph is written back: its t is the entry's bit for bit, its q the entry's as the write-back normalises it, bit
    for bit (on the CPU executor 16 of the 48 components differ from the entry's, by 2.2e-16 at most, so "equal to
    the entry bit for bit" is not what the documented write-back gives)."""
    sc, ref = scene(name), reference(name)
    print(name, {k: out[k] for k in ("status", "termination", "ok", "num_iterations", "num_successful_steps",
                                     "num_unsuccessful_steps", "num_invalid_steps", "initial_cost", "final_cost")})
    print(name, "the reference:", {k: ref[k] for k in ("termination", "ok", "num_iterations", "num_successful_steps",
                                                       "num_unsuccessful_steps", "num_invalid_steps", "initial_cost")})
    assert out["status"] == ("OK" if ref["ok"] else "FAILED") and out["ok"] == ref["ok"]
    assert out["termination"] == ref["termination"]
    for key in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps"):
        assert out[key] == ref[key], (key, out[key], ref[key])
    assert abs(out["initial_cost"] - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
    if name == "maxiter_chords24":
        d = compare(states(m, np.arange(len(sc["q"])), out["log_scale"]), ref["x"])
        d["cost"] = abs(out["final_cost"] - ref["final_cost"])
        print(name, "against the reference after two steps:", d, "bounds:", {k: bound(name, k) for k in d})
        for key, val in d.items():
            assert val <= bound(name, key), (key, val, bound(name, key))
    else:
        # no step was accepted (FAILED, or the radius test after rejected steps): nothing moved, bit for bit
        assert ref["num_successful_steps"] == 0
        want_q = before.q if not ref["ok"] else written_back_q(before.q.reshape(-1, 4), sc["fixed"]).reshape(-1)
        print(name, "q components that differ from the entry's:", int((m.q != before.q).sum()), "by at most",
              float(np.abs(m.q - before.q).max()))
        assert m.q.tobytes() == want_q.tobytes() and m.t.tobytes() == before.t.tobytes()
        assert np.abs(m.q - before.q).max() <= 2.0 * EPS
        assert (out["log_scale"] == 0.0).all()
        assert abs(out["final_cost"] - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]


# ---------------------------------------------------------------------------------------------- measurements
def pose_edges_np(q, t, pairs, sim=None):
    """sg_map_pose_edges in numpy: (n, 8)."""
    out = np.zeros((len(pairs), 8))
    for i, (a, b) in enumerate(pairs):
        qa, ta, s = qunit(q[a]), np.array(t[a], float), 1.0
        if sim is not None:
            s, qs, ts = float(sim[0]), qunit(sim[1]), np.asarray(sim[2], float)
            ta = s * quat_to_matrix(qs) @ ta + ts
            qa = qunit(qmul(qa, qconj(qs)))
        out[i, :4] = qunit(qmul(qa, qconj(qunit(q[b]))))
        out[i, 4:7] = quat_to_matrix(qa) @ (np.asarray(t[b], float) - ta) / s
        out[i, 7] = -np.log(s) if sim is not None else 0.0
    return out


def frames_map(q, t):
    """A map that holds frames only."""
    F = len(q)
    z = np.zeros(0)
    zi = np.zeros(0, dtype=np.int32)
    return MapArrays(k=np.tile([0.0, 0.0, 0.0, 500.0, 500.0, 320.0, 240.0], 2), q=np.array(q, float).reshape(-1),
                     t=np.array(t, float).reshape(-1), frame_camera=np.zeros(F, dtype=np.int32),
                     frame_prev=(np.arange(F) - 1).astype(np.int32), X=z.copy(), point_flags=zi.copy(),
                     point_uncertainty=z.copy(), obs_pt=z.copy(), obs_frame=zi.copy(), obs_point=zi.copy(),
                     obs_disabled=zi.copy(), obs_error=z.copy())


def graph_of(sc, frames=None):
    """The scene as OptimizePoseGraph takes it (node i is map frame frames[i], by default i)."""
    N = len(sc["q"])
    return {"frames": np.arange(N) if frames is None else frames, "fixed": sc["fixed"], "edges": sc["edges"],
            "meas": sc["meas"], "weights": sc["weights"]}


def host_slam():
    """A Slam facade without a handle: for its host-only methods (no device is touched)."""
    from slamgpu.ba import Slam
    from slamgpu.capi import load_library
    s = Slam.__new__(Slam)
    s.lib, s.h = load_library(), None
    return s


# ---------------------------------------------------------------------------------------------- scenes
def _circle(N, radius, rng, wobble=0.15):
    """Poses on a circle in the x-z plane, looking along the tangent, with a seeded wobble."""
    q, t = np.zeros((N, 4)), np.zeros((N, 3))
    for i in range(N):
        a = 2.0 * np.pi * i / N
        t[i] = [radius * np.cos(a), 40.0 * np.sin(3 * a), radius * np.sin(a)]
        yaw = np.array([0.0, -a, 0.0])
        q[i] = quat_from_matrix(axis_angle(rng.normal(size=3) * wobble) @ axis_angle(yaw))
    return q, t


def _perturbed(q, t, fixed, rng, rot_deg, trans):
    q0, t0 = q.copy(), t.copy()
    for i in range(len(q)):
        if fixed[i]:
            continue
        q0[i] = quat_from_matrix(axis_angle(rng.normal(size=3) / np.sqrt(3) * np.radians(rot_deg)) @ quat_to_matrix(q[i]))
        t0[i] = t[i] + rng.normal(0.0, trans, size=3)
    return q0, t0


def _weights(E):
    return np.tile([W_ROT, W_T, W_S], (E, 1))


def _exact(name, N, edges, fixed_nodes, seed, radius=1000.0, rot_deg=2.0, trans=20.0):
    rng = np.random.default_rng(seed)
    q, t = _circle(N, radius, rng)
    fixed = np.zeros(N, dtype=np.int32)
    fixed[list(fixed_nodes)] = 1
    edges = np.array(edges, dtype=np.int32)
    q0, t0 = _perturbed(q, t, fixed, rng, rot_deg, trans)
    return dict(name=name, q=q0, t=t0, fixed=fixed, edges=edges, meas=pose_edges_np(q, t, edges),
                weights=_weights(len(edges)), range=0.0, fix_scale=False, q_true=q, t_true=t)


def _drift12():
    """A 12-node ring whose map drifted: every odometry step carries a small extra rotation, a translation bias and a
    scale error that accumulates; the odometry edges are measured from the drifted map as it stands (zero residual at
    entry), and the loop edge 11 -> 0 comes through the similarity path: the similarity that takes the drifted frame 11
    onto its true pose, at the scale its piece of the map has drifted to."""
    rng = np.random.default_rng(12)
    N = 12
    q, t = _circle(N, 1000.0, rng)
    R = [quat_to_matrix(x) for x in q]
    Rd, td, lam = [R[0]], [t[0].copy()], [1.0]
    for i in range(N - 1):
        Rrel = R[i + 1] @ R[i].T
        u = R[i] @ (t[i + 1] - t[i])
        lam.append(lam[-1] * 1.012)
        td.append(td[-1] + Rd[-1].T @ (lam[-1] * u + np.array([1.5, -0.8, 1.0])))
        Rd.append(axis_angle(np.radians([0.25, 0.4, -0.15])) @ Rrel @ Rd[-1])
    qd = np.stack([quat_from_matrix(x) for x in Rd])
    td = np.stack(td)
    odo = np.array([[i, i + 1] for i in range(N - 1)], dtype=np.int32)
    s = 1.0 / lam[-1]
    RS = R[-1].T @ Rd[-1]
    sim = (s, quat_from_matrix(RS), t[-1] - s * RS @ td[-1])
    # frame 0 of the drifted map is the true one, so the loop edge's b side is the truth
    loop = pose_edges_np(np.vstack([qd[:-1], qd[-1:]]), td, [(N - 1, 0)], sim)
    fixed = np.zeros(N, dtype=np.int32)
    fixed[0] = 1
    edges = np.vstack([odo, [[N - 1, 0]]]).astype(np.int32)
    meas = np.vstack([pose_edges_np(qd, td, odo), loop])
    return dict(name="drift12", q=qd, t=td, fixed=fixed, edges=edges, meas=meas, weights=_weights(len(edges)),
                range=0.0, fix_scale=False, q_true=q, t_true=t, sim=sim)


def scene(name):
    if name in _cache:
        return _cache[name]
    if name == "ring8":
        sc = _exact(name, 8, [(i, (i + 1) % 8) for i in range(8)], [0], 8)
    elif name == "drift12":
        sc = _drift12()
    elif name == "chords24":
        rng = np.random.default_rng(24)
        ed = [(i, (i + 1) % 24) for i in range(24)]
        while len(ed) < 34:
            a, b = (int(v) for v in rng.integers(0, 24, size=2))
            if a != b and (a, b) not in ed and (b, a) not in ed:
                ed.append((a, b))
        sc = _exact(name, 24, ed, [0, 5], 24)
    elif name == "rigid12":
        sc = dict(scene("drift12"), name=name, fix_scale=True)
    elif name == "badloop12":
        base = scene("drift12")
        wrong = np.concatenate([qunit([0.3, -0.5, 0.2, 0.6]), [400.0, -300.0, 250.0], [0.5]])
        sc = dict(base, name=name, edges=np.vstack([base["edges"], [[3, 8]]]).astype(np.int32),
                  meas=np.vstack([base["meas"], wrong]), weights=_weights(len(base["edges"]) + 1), range=BAD_RANGE)
    elif name == "long300":
        N = 300
        ed = [(i, i + k) for i in range(N) for k in (1, 2, 3) if i + k < N]
        ed += [(299, 0), (250, 40), (200, 75), (150, 10), (280, 120)]
        sc = _exact(name, N, ed, [0], 300, radius=4000.0, rot_deg=1.0, trans=10.0)
    elif name == "far12":
        # a start far outside the basin (120 degrees, 1500 map units on a circle of radius 1000): LM rejects steps
        sc = _exact(name, 12, [(i, (i + 1) % 12) for i in range(12)], [0], 112, rot_deg=120.0, trans=1500.0)
    elif name == "farrigid12":
        # the same with fix_scale, on a seed of its own: far12's start ends within a factor 2 of the gradient
        # tolerance when the scale is fixed, which the reference-bounds test does not allow
        sc = _exact(name, 12, [(i, (i + 1) % 12) for i in range(12)], [0], 137, rot_deg=120.0, trans=1500.0)
        sc["fix_scale"] = True
    elif name == "farcauchy12":
        sc = dict(scene("far12"), name=name, range=BAD_RANGE)
    elif name == "minradius_far12":
        sc = dict(scene("far12"), name=name)
    elif name == "maxiter_chords24":
        sc = dict(scene("chords24"), name=name)
    elif name == "complete48":
        # every pair an edge: the column eliminated j-th has 46 - j off-diagonal blocks, so the first ten columns
        # give the strided loops over rows * D items (up to 322) a second trip
        sc = _exact(name, 48, [(a, b) for a in range(48) for b in range(a + 1, 48)], [0], 148)
    elif name == "star40":
        # a free hub of 39 edges, a leaf fixed: one block and one gradient segment gather 39 contributions
        sc = _exact(name, 40, [(0, b) for b in range(1, 40)], [1], 141)
    elif name in LOOSE_NODE:
        members = [0, 2, 3, 4, 5, 6, 7, 8] if name == "loose_first9" else list(range(8))
        ring = [(members[i], members[(i + 1) % 8]) for i in range(8)]
        loose = {"loose_first9": [(4, 1)], "loose_last9": [(i, 8) for i in range(8)]}.get(name, [(3, 8)])
        sc = _exact(name, 9, ring + loose, [0], 109)
        sc["weights"][len(ring):] = LOOSE_W
    elif name == "cap1024":
        # the node cap (kPgMaxNodes): long300's construction, edges to the next 3 nodes and five long chords
        N = 1024
        ed = [(i, i + k) for i in range(N) for k in (1, 2, 3) if i + k < N]
        ed += [(1023, 0), (850, 140), (700, 260), (500, 30), (960, 410)]
        sc = _exact(name, N, ed, [0], 1029, radius=12000.0, rot_deg=1.0, trans=10.0)
    elif name == "two_comp":
        a = _exact("a", 6, [(i, (i + 1) % 6) for i in range(6)], [0], 61)
        b = _exact("b", 5, [(i, (i + 1) % 5) for i in range(5)], [], 62)
        sc = dict(name=name, q=np.vstack([a["q"], b["q"]]), t=np.vstack([a["t"], b["t"] + 5000.0]),
                  fixed=np.concatenate([a["fixed"], b["fixed"]]), edges=np.vstack([a["edges"], b["edges"] + 6]),
                  meas=np.vstack([a["meas"], b["meas"]]), weights=_weights(11), range=0.0, fix_scale=False)
    else:
        raise KeyError(name)
    _cache[name] = sc
    return sc


# ---------------------------------------------------------------------------------------------- the loop-closing scene
LOOP_CLOSING = (8, 9)            # the frames that re-observe old landmarks
LOOP_W = 10.0                    # a loop edge's weights over an odometry edge's
LOOP_THRESHOLD = 60.0            # AlignPoints' threshold: the joint fit of both closing frames is not exact


def _compose(A, B):
    """The similarity A after B, each (s, R, t)."""
    return A[0] * B[0], A[1] @ B[1], A[0] * A[1] @ B[2] + A[2]


def loop_scene():
    """C1 at its true poses and points; its second half (frames 4 .. 9) carries a planted smooth drift: frame f is
    moved by S1^(f - 3), S1 a similarity of scale 1.01, 0.46 degrees and 5.4 map units, and so is every point first
    seen from it.  The closing frames 8 and 9 each re-observe 40 landmarks of the undrifted beginning, which the map
    holds a second time: as new points triangulated from that frame, in its drifted coordinates.  Returns the map,
    the truth, per closing frame the (new, old) correspondences, the frames and points of the drifted piece and the
    odometry pairs."""
    if "loop" in _cache:
        return _cache["loop"]
    from slamgpu.scene import make_config, project_np
    m = make_config("C1", perturb=False)
    F, P = m.num_frames, m.num_points
    q_true, t_true = m.q.reshape(-1, 4).copy(), m.t.reshape(-1, 3).copy()
    X = m.X.reshape(-1, 4)
    Xe = X[:, :3] / X[:, 3:]
    anchor = np.full(P, -1)
    for f, p in zip(m.obs_frame, m.obs_point):
        if anchor[p] < 0:
            anchor[p] = f
    S1 = (1.01, axis_angle(np.radians([0.1, 0.4, -0.2])), np.array([3.0, -2.0, 4.0]))
    S = [(1.0, np.eye(3), np.zeros(3))]
    for _ in range(F):
        S.append(_compose(S1, S[-1]))
    drift = lambda f: S[max(f - 3, 0)]
    q, t = q_true.copy(), t_true.copy()
    for f in range(4, F):
        s, R, tt = drift(f)
        t[f] = s * R @ t_true[f] + tt
        q[f] = quat_from_matrix(quat_to_matrix(q_true[f]) @ R.T)
    Xd = np.stack([drift(a)[0] * drift(a)[1] @ x + drift(a)[2] for a, x in zip(anchor, Xe)])
    rng = np.random.default_rng(89)
    old = rng.permutation(np.flatnonzero((anchor >= 0) & (anchor <= 3)))
    groups, new_X, new_obs = {}, [], []
    for i, c in enumerate(LOOP_CLOSING):
        pick = old[40 * i:40 * i + 40]
        s, R, tt = drift(c)
        ids = P + len(new_X) + np.arange(len(pick))
        groups[c] = np.stack([ids, pick], 1).astype(np.int32)
        new_X += [s * R @ Xe[p] + tt for p in pick]
        uv, _ = project_np(np.tile(quat_to_matrix(q_true[c]), (len(pick), 1, 1)), np.tile(t_true[c], (len(pick), 1)),
                           m.k[:7], Xe[pick])
        new_obs += [(c, pid, px) for pid, px in zip(ids, uv)]
    allX = np.vstack([Xd, np.array(new_X)])
    Xh = np.concatenate([allX, np.ones((len(allX), 1))], 1)
    Xh /= np.linalg.norm(Xh, axis=1, keepdims=True)
    n_new = len(new_X)
    mm = MapArrays(
        k=m.k, q=q.reshape(-1).copy(), t=t.reshape(-1).copy(), frame_camera=m.frame_camera, frame_prev=m.frame_prev,
        X=Xh.reshape(-1).copy(), point_flags=np.zeros(P + n_new, dtype=np.int32), point_uncertainty=np.ones(P + n_new),
        obs_pt=np.concatenate([m.obs_pt, np.array([o[2] for o in new_obs]).reshape(-1)]),
        obs_frame=np.concatenate([m.obs_frame, [o[0] for o in new_obs]]).astype(np.int32),
        obs_point=np.concatenate([m.obs_point, [o[1] for o in new_obs]]).astype(np.int32),
        obs_disabled=np.zeros(m.num_obs + n_new, dtype=np.int32), obs_error=np.zeros(2 * (m.num_obs + n_new)))
    piece_points = np.concatenate([np.flatnonzero(anchor >= 4), P + np.arange(n_new)]).astype(np.int32)
    odo = np.array([(i, i + 1) for i in range(F - 1)] + [(i, i + 2) for i in range(F - 2)], dtype=np.int32)
    fixed = np.zeros(F, dtype=np.int32)
    fixed[:2] = 1
    _cache["loop"] = dict(map=mm, q_true=q_true, t_true=t_true, groups=groups, piece_frames=np.arange(4, F, dtype=np.int32),
                          piece_points=piece_points, odo=odo, fixed=fixed)
    return _cache["loop"]


def loop_graph(ls, odo_meas, loop_meas):
    """The graph of the loop-closing scene: the odometry edges as measured, then one loop edge per closing frame to
    frame 0, LOOP_W times as heavy."""
    edges = np.vstack([ls["odo"], [[c, 0] for c in LOOP_CLOSING]]).astype(np.int32)
    w = np.vstack([_weights(len(ls["odo"])), LOOP_W * _weights(len(LOOP_CLOSING))])
    return {"frames": np.arange(len(ls["fixed"])), "fixed": ls["fixed"], "edges": edges,
            "meas": np.vstack([odo_meas, loop_meas]), "weights": w}


def closing_errors(ls, q, t):
    """Worst pose error of the closing frames against the truth: (rotation deg, centre in map units)."""
    q, t = np.asarray(q).reshape(-1, 4), np.asarray(t).reshape(-1, 3)
    return (max(rot_err_deg(qunit(q[c]), qunit(ls["q_true"][c])) for c in LOOP_CLOSING),
            max(float(np.linalg.norm(t[c] - ls["t_true"][c])) for c in LOOP_CLOSING))


def loop_reference():
    """The chain in numpy: Horn's similarity per closing frame and over both (align_cases.horn_np), the loop edges, the
    reference solve; returns the closing frames' errors after the one rigid similarity and after the pose graph."""
    if "loop_ref" in _cache:
        return _cache["loop_ref"]
    import align_cases as ac
    ls = loop_scene()
    m = ls["map"]
    q, t = m.q.reshape(-1, 4), m.t.reshape(-1, 3)
    Xe = m.X.reshape(-1, 4)[:, :3] / m.X.reshape(-1, 4)[:, 3:]
    horn = lambda corr: ac.horn_np(Xe[corr[:, 0]], Xe[corr[:, 1]])[:3]
    loop_meas = []
    for c in LOOP_CLOSING:
        s, R, tt = horn(ls["groups"][c])
        loop_meas.append(pose_edges_np(q, t, [(c, 0)], (s, quat_from_matrix(R), tt))[0])
    s, R, tt = horn(np.vstack([ls["groups"][c] for c in LOOP_CLOSING]))
    qr, tr = q.copy(), t.copy()
    for f in ls["piece_frames"]:
        tr[f] = s * R @ t[f] + tt
        qr[f] = quat_from_matrix(quat_to_matrix(q[f]) @ R.T)
    g = loop_graph(ls, pose_edges_np(q, t, ls["odo"]), np.array(loop_meas))
    sc = dict(q=q, t=t, fixed=g["fixed"], edges=g["edges"], meas=g["meas"], weights=g["weights"], range=0.0,
              fix_scale=False)
    ref = solve_np(sc)
    _cache["loop_ref"] = dict(rigid=closing_errors(ls, qr, tr), graph=closing_errors(ls, ref["x"][:, :4], ref["x"][:, 4:7]),
                              ref=ref, scene=sc)
    return _cache["loop_ref"]
