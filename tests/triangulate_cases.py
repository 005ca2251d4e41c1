"""Inputs, the numpy reference and the comparison bounds shared by the triangulation tests
(test_triangulate_reference_bounds.py on the CPU, test_triangulate_gpu.py on the device).

The comparator is always triangulate_np below: a numpy restatement of the seven steps of
sg_slam_triangulate_points (include/slamgpu.h) with np.linalg.eigh (LAPACK) for the eigen-solve.  It shares no code
with the library.

Bounds.  The reference against itself, with a point's records summed forward and reversed (c0 and L kept), moves by
the SPREAD_* values below on scenes A and B, noisy and exact (test_triangulate_reference_bounds.py recomputes them
and checks they are not exceeded).  The eigenvector's sensitivity is inversely proportional to the eigen gap, so X
is compared both raw and weighted by rel_gap.  The device differs from the reference in algorithm (Jacobi rotations
against LAPACK, the 8-lane summation order, FMA contraction), not only in order, so its bounds are 100 x the
spreads."""
import numpy as np

import points_cases as pc
from slamgpu.scene import make_config, make_scene, project_np, quat_to_matrix

MIN_OBS = 2            # kPointMinObs
MIN_REL_GAP = 1e-12    # kTriMinRelGap

# the reference alone, forward against reversed summation (worst over scenes A and B, noisy and exact)
SPREAD_X_GAP = 1.0e-15       # |dX|_2 * rel_gap
SPREAD_X = 1.2e-14           # |dX|_2 (X has unit 4-norm)
SPREAD_ERROR_PX = 2.0e-12    # max_error_px
SPREAD_PARALLAX = 8.0e-15    # rad
SPREAD_REL_GAP = 8.0e-16     # rel_gap, absolute
MARGIN = 100.0
EXACT_ERROR_PX = 1e-9        # exact scenes: max_error_px of every point (the reference alone: 2.2e-12 px)
GATE_PX, GATE_RAD = 5.0, np.deg2rad(1.0)
NEAR_GATE = 1e-6             # px, rad: a point this close to a gate may fall on either side
NEAR_GATE_POINTS = 0         # such points allowed (none exist: the nearest are 0.255 px and 0.0036 deg away)

_cache = {}


def scene(name, exact=False):
    """Scene A or B of points_cases with every frame at its true pose; exact: noise-free observations."""
    key = ("tri", name, exact)
    if key not in _cache:
        if exact:
            kw = dict(noise=0.0, outlier_frac=0.0, perturb=False)
            m = make_config("C1", **kw) if name == "A" else make_scene(40, 400, 7, run_max=40, **kw)
        else:
            m = pc.scene(name)
        m.q[:] = m.q_true
        m.t[:] = m.t_true
        _cache[key] = m
    return _cache[key].copy()


def distorted_scene():
    """Scene A exact with both cameras' k = (-0.1, 0.02, 0, ...) and the observations regenerated from the truth
    through project_np."""
    m = scene("A", exact=True)
    m.k[0:3] = m.k[7:10] = (-0.1, 0.02, 0.0)
    Xt = m.X_true.reshape(-1, 4)
    Xw = (Xt[:, :3] / Xt[:, 3:])[m.obs_point]
    R = np.stack([quat_to_matrix(q) for q in m.q.reshape(-1, 4)])[m.obs_frame]
    uv, ok = project_np(R, m.t.reshape(-1, 3)[m.obs_frame], m.k[:7], Xw)
    assert ok.all()
    m.obs_pt[:] = uv.reshape(-1)
    return m


def undistort_np(k, pt):
    xd, yd = (pt[0] - k[5]) / k[3], (pt[1] - k[6]) / k[4]
    rd = np.hypot(xd, yd)
    if rd == 0:
        return 0.0, 0.0
    r = rd
    for _ in range(8):
        r2 = r * r
        f = r * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) - rd
        df = 1 + r2 * (3 * k[0] + r2 * (5 * k[1] + r2 * 7 * k[2]))
        r = r - f / df
    return xd * r / rd, yd * r / rd


def project_one(R, t, k, X):
    """project.h on a homogeneous X: (uv, in front)."""
    p = R @ (X[:3] - t * X[3])
    if p[2] < 0.001 * X[3]:
        return None, False
    xp, yp = p[0] / p[2], p[1] / p[2]
    r2 = xp * xp + yp * yp
    d = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
    return np.array([xp * d * k[3] + k[5], yp * d * k[4] + k[6]]), True


def triangulate_np(m, p, min_parallax=0.0, max_error_px=0.0, reverse=False):
    """The seven steps for point p of m: dict(status, num_obs, parallax, max_error_px, rel_gap, X).  reverse: the
    sums over the records run backwards (c0 stays the first record's centre)."""
    sel = pc.enabled_obs(m, p)
    n = len(sel)
    out = dict(status="DID_NOT_RUN", num_obs=n, parallax=0.0, max_error_px=0.0, rel_gap=0.0, X=np.zeros(4))
    if n < MIN_OBS:
        return out
    fr = m.obs_frame[sel]
    t = m.t.reshape(-1, 3)[fr]
    R = [quat_to_matrix(m.q[4 * f:4 * f + 4]) for f in fr]
    K = [m.k[7 * m.frame_camera[f]:7 * m.frame_camera[f] + 7] for f in fr]
    pts = m.obs_pt.reshape(-1, 2)[sel]
    order = range(n - 1, -1, -1) if reverse else range(n)
    c0 = t[0]
    L2 = 0.0
    for i in order:
        L2 += float(np.dot(t[i] - c0, t[i] - c0))
    L2 /= n
    if L2 == 0.0:
        out["status"] = "NO_BASELINE"
        return out
    L = np.sqrt(L2)
    M = np.zeros((4, 4))
    for i in order:
        a, b = undistort_np(K[i], pts[i])
        c = (t[i] - c0) / L
        for nrm in (a * R[i][2] - R[i][0], b * R[i][2] - R[i][1]):
            row = np.append(nrm, -np.dot(nrm, c))
            M += np.outer(row, row)
    if not np.isfinite(M).all():
        out["status"] = "DEGENERATE"
        return out
    lam, V = np.linalg.eigh(M)
    y = V[:, 0] / np.linalg.norm(V[:, 0])
    if not (lam[1] - lam[0] > MIN_REL_GAP * lam[3]):
        out["status"] = "DEGENERATE"
        return out
    out["rel_gap"] = (lam[1] - lam[0]) / lam[3]
    X = np.append(L * y[:3] + c0 * y[3], y[3])
    if X[3] < 0 or (X[3] == 0 and (R[0] @ X[:3])[2] < 0):
        X = -X
    X /= np.linalg.norm(X)
    behind, err, par = 0, 0.0, 0.0
    d0 = X[:3] - t[0] * X[3]
    for i in order:
        uv, ok = project_one(R[i], t[i], K[i], X)
        if ok:
            err = max(err, float(np.hypot(*(uv - pts[i]))))
        else:
            behind += 1
        d = X[:3] - t[i] * X[3]
        par = max(par, float(np.arctan2(np.linalg.norm(np.cross(d, d0)), np.dot(d, d0))))
    out.update(X=X, parallax=par, max_error_px=err)
    if behind:
        out["status"] = "BEHIND"
    elif min_parallax != 0 and par < min_parallax:
        out["status"] = "LOW_PARALLAX"
    elif max_error_px != 0 and err > max_error_px:
        out["status"] = "HIGH_ERROR"
    else:
        out["status"] = "OK"
    return out


def reference(name, exact=False, gates=False, reverse=False):
    """triangulate_np on every point of the scene, computed once and left unchanged."""
    key = ("ref", name, exact, gates, reverse)
    if key not in _cache:
        m = scene(name, exact)
        g = (GATE_RAD, GATE_PX) if gates else (0.0, 0.0)
        _cache[key] = [triangulate_np(m, p, g[0], g[1], reverse) for p in range(m.num_points)]
    return _cache[key]


def spreads(res, ref):
    """Worst differences between two result lists over the points both computed: dict of the SPREAD_* rows."""
    w = dict(x_gap=0.0, x=0.0, error_px=0.0, parallax=0.0, rel_gap=0.0)
    for a, b in zip(res, ref):
        if not (np.any(a["X"]) and np.any(b["X"])):
            continue
        dx = float(np.linalg.norm(a["X"] - b["X"]))
        w["x"] = max(w["x"], dx)
        w["x_gap"] = max(w["x_gap"], dx * b["rel_gap"])
        w["error_px"] = max(w["error_px"], abs(a["max_error_px"] - b["max_error_px"]))
        w["parallax"] = max(w["parallax"], abs(a["parallax"] - b["parallax"]))
        w["rel_gap"] = max(w["rel_gap"], abs(a["rel_gap"] - b["rel_gap"]))
    return w


LIMITS = dict(x_gap=SPREAD_X_GAP, x=SPREAD_X, error_px=SPREAD_ERROR_PX, parallax=SPREAD_PARALLAX,
              rel_gap=SPREAD_REL_GAP)


def compare(label, res, ref, margin=MARGIN):
    """Prints the worst value of every row, then asserts margin x the reference's own spread."""
    w = spreads(res, ref)
    print("%s, %d points: |dX| rel_gap %.2e; |dX| %.2e; max_error_px %.2e; parallax %.2e rad; rel_gap %.2e" % (
        label, len(ref), w["x_gap"], w["x"], w["error_px"], w["parallax"], w["rel_gap"]))
    for row, limit in LIMITS.items():
        assert w[row] <= margin * limit, (row, w[row], margin * limit)
    return w
