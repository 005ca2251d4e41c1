"""Shared inputs and numpy references of the localization tests (sg_slam_localize_frames).

Scenes come from make_config("C1") with the true poses of the listed frames kept aside:
  exact: noise=0, outlier_frac=0, perturb=False (so X = X_true and every pixel is the projection of its point);
  noisy: the stock 0.5 px pixel noise, also with outlier_frac=0 and perturb=False: the outliers are the planted
         ones only, so the expected inlier mask is known.
plant_outliers replaces a share of one frame's records by pixels uniform in the image and at least 20 px from the
true projection.  garbage_pose overwrites the entry pose of the listed frames.

The references are restated here in numpy and are never another path of the library: the sampler (sample_np, the
hash of include/slamgpu.h), a P3P by Newton on the three distance equations from the true depths followed by
Horn/Kabsch with np.linalg.svd (p3p_newton_np), the projection and the MSAC scorer (project_np_q, score_np)."""
import numpy as np

from slamgpu.scene import HEIGHT, WIDTH, make_config, quat_from_matrix, quat_to_matrix

TAU = 4.0                   # threshold_px of every test
MIN_OUTLIER_PX = 20.0       # planted outliers are at least this far from the true projection
NEAR = 1e-6                 # no record of a test frame may lie this close to TAU at the reference optimum
UNUSABLE = (1 << 0) | (1 << 1) | (1 << 2) | (1 << 4)   # BAD_LOCATION, NO_BASELINE, NO_OBSERVATIONS, BAD_FEATURE
FRAMES = (3, 8)             # the C1 frames the tests localize
PNP_MIN_W = 1e-9            # kPnpMinW of csrc/pnp_math.h

# Worst inlier reprojection error (px) of p3p_newton_np's pose on the exact scenes, from the well-spread sample of
# spread_sample(), over FRAMES: recomputed by tests/test_localize_reference_bounds.py, which fails when this value is
# not an upper bound within a factor of 4.  The device gets MARGIN times it: another algorithm (closed form, triads
# instead of an SVD), another summation order and FMA contraction, as the triangulation tests argue.
SPREAD_EXACT_PX = 2e-12
MARGIN = 100.0

_M32 = 0xFFFFFFFF
_cache = {}


# ---------------------------------------------------------------------------------------------- sampler
def mix(x: int) -> int:
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def sample_np(seed: int, f: int, h: int, n: int) -> tuple:
    """Hypothesis h of map frame f over n records: three distinct indices (include/slamgpu.h, step 2)."""
    base = mix(mix(mix(seed) + f) + h)
    r = [mix(base ^ ((0x9E3779B9 * (j + 1)) & _M32)) for j in range(3)]
    i0, i1, i2 = (r[0] * n) >> 32, (r[1] * (n - 1)) >> 32, (r[2] * (n - 2)) >> 32
    if i1 >= i0:
        i1 += 1
    lo, hi = min(i0, i1), max(i0, i1)
    if i2 >= lo:
        i2 += 1
    if i2 >= hi:
        i2 += 1
    return i0, i1, i2


# ---------------------------------------------------------------------------------------------- projection, score
def project_np_q(q, t, k, X):
    """project.h on homogeneous points X (n, 4) at the pose (q, t): pixels (n, 2) and the accepted mask."""
    R = quat_to_matrix(np.asarray(q, dtype=np.float64))
    v = X[:, :3] - np.asarray(t)[None, :] * X[:, 3:4]
    p = v @ R.T
    ok = ~(p[:, 2] < 0.001 * X[:, 3])
    z = np.where(ok, p[:, 2], 1.0)
    xp, yp = p[:, 0] / z, p[:, 1] / z
    r2 = xp * xp + yp * yp
    d = 1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
    return np.stack([k[3] * d * xp + k[5], k[4] * d * yp + k[6]], 1), ok


def score_np(q, t, k, X, pt, tau=TAU):
    """Pixel errors e (inf where the projection refuses the record), the inlier mask e^2 <= tau^2 and the MSAC cost
    sum min(e^2, tau^2)."""
    uv, ok = project_np_q(q, t, k, X)
    with np.errstate(invalid="ignore", over="ignore"):
        e2 = ((uv - pt) ** 2).sum(1)
    e2 = np.where(ok & np.isfinite(e2), e2, np.inf)
    inl = e2 <= tau * tau
    return np.sqrt(e2), inl, float(np.where(inl, e2, tau * tau).sum())


def bearings_np(k, pt):
    """Pixels (n, 2) -> unit bearings (n, 3): the radial distortion inverted by Newton on the radius."""
    xd, yd = (pt[:, 0] - k[5]) / k[3], (pt[:, 1] - k[6]) / k[4]
    rd = np.hypot(xd, yd)
    r = rd.copy()
    for _ in range(20):
        r2 = r * r
        fr = r * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) - rd
        df = 1 + r2 * (3 * k[0] + r2 * (5 * k[1] + r2 * 7 * k[2]))
        r = r - fr / df
    s = np.where(rd > 0, r / np.where(rd > 0, rd, 1.0), 0.0)
    b = np.stack([xd * s, yd * s, np.ones_like(xd)], 1)
    return b / np.linalg.norm(b, axis=1, keepdims=True)


def p3p_newton_np(f, P, s0):
    """Reference P3P: Newton on the three distance equations |s_i f_i - s_j f_j|^2 = |P_i - P_j|^2 from the depths
    s0, then the rigid motion Y_i = R (P_i - C) by Horn/Kabsch (np.linalg.svd).  Returns (q, C)."""
    f, P, s = np.asarray(f, float), np.asarray(P, float), np.asarray(s0, float).copy()
    pairs = ((1, 2), (0, 2), (0, 1))
    d2 = np.array([((P[i] - P[j]) ** 2).sum() for i, j in pairs])
    c = np.array([f[i] @ f[j] for i, j in pairs])
    for _ in range(20):
        g = np.array([s[i] ** 2 + s[j] ** 2 - 2 * s[i] * s[j] * c[n] - d2[n] for n, (i, j) in enumerate(pairs)])
        J = np.zeros((3, 3))
        for n, (i, j) in enumerate(pairs):
            J[n, i] = 2 * (s[i] - s[j] * c[n])
            J[n, j] = 2 * (s[j] - s[i] * c[n])
        step = np.linalg.solve(J, g)
        s -= step
        if np.abs(step).max() <= 1e-15 * np.abs(s).max():
            break
    Y = s[:, None] * f
    ym, pm = Y.mean(0), P.mean(0)
    U, _, Vt = np.linalg.svd((Y - ym).T @ (P - pm))
    # three points span a plane: the third singular direction carries the sign that makes det R = +1
    D = np.diag([1.0, 1.0, np.linalg.det(U @ Vt)])
    R = U @ D @ Vt
    return quat_from_matrix(R), pm - R.T @ ym


# ---------------------------------------------------------------------------------------------- scenes
def usable_obs(m, f):
    return np.flatnonzero((m.obs_frame == f) & (m.obs_disabled == 0) & ((m.point_flags[m.obs_point] & UNUSABLE) == 0))


def frame_records(m, f):
    """(obs indices, pixels (n, 2), points (n, 4), intrinsics) of frame f's records, in map order."""
    sel = usable_obs(m, f)
    k = m.k[7 * m.frame_camera[f]:7 * m.frame_camera[f] + 7]
    return sel, m.obs_pt.reshape(-1, 2)[sel], m.X.reshape(-1, 4)[m.obs_point[sel]], k


def base_scene(kind: str):
    """'exact' or 'noisy' C1, entry poses still the truth.  A fresh copy per call."""
    if kind not in _cache:
        kw = dict(outlier_frac=0.0, perturb=False)
        if kind == "exact":
            kw["noise"] = 0.0
        else:
            assert kind == "noisy"
        m = make_config("C1", **kw)
        assert np.array_equal(m.X, m.X_true) and np.array_equal(m.q, m.q_true) and np.array_equal(m.t, m.t_true)
        _cache[kind] = m
    return _cache[kind].copy()


def true_pose(m, f):
    return m.q_true[4 * f:4 * f + 4].copy(), m.t_true[3 * f:3 * f + 3].copy()


def plant_outliers(m, f, share: float, seed: int):
    """Replaces round(share * N) of frame f's records (chosen by the seeded generator) by pixels uniform in the image
    and at least MIN_OUTLIER_PX from the true projection.  Returns the planted mask over the frame's records."""
    sel, _, X, k = frame_records(m, f)
    rng = np.random.default_rng(seed)
    n = len(sel)
    out = np.zeros(n, dtype=bool)
    out[rng.choice(n, size=int(round(share * n)), replace=False)] = True
    uv, ok = project_np_q(*true_pose(m, f), k, X)
    assert ok.all()
    pts = m.obs_pt.reshape(-1, 2)
    for j in np.flatnonzero(out):
        while True:
            p = rng.uniform((0.0, 0.0), (WIDTH, HEIGHT))
            if np.hypot(*(p - uv[j])) >= MIN_OUTLIER_PX:
                break
        pts[sel[j]] = p
    return out


def garbage_pose(m, frames):
    """The entry pose of the listed frames becomes garbage: looking the other way, 100 m off."""
    for f in frames:
        m.q[4 * f:4 * f + 4] = (0.5, -0.5, 0.5, 0.5)
        m.t[3 * f:3 * f + 3] = (1e5, -2e5, 3e5)


def scene(kind: str, share: float, frames=FRAMES, garbage: bool = True):
    """The scene `kind` with `share` outliers planted in each listed frame (seed 100 + f) and, by default, a garbage
    entry pose.  Returns (map, {f: planted-outlier mask over f's records})."""
    m = base_scene(kind)
    masks = {f: plant_outliers(m, f, share, 100 + f) for f in frames}
    if garbage:
        garbage_pose(m, frames)
    return m, masks


def spread_sample(pt):
    """The fixed, well-spread sample of the reference bound: the records nearest to three image positions, left-top
    (80, 60), right-top (560, 60) and bottom-centre (320, 420)."""
    anchors = np.array([(80.0, 60.0), (560.0, 60.0), (320.0, 420.0)])
    idx = [int(np.argmin(((pt - a) ** 2).sum(1))) for a in anchors]
    assert len(set(idx)) == 3
    return idx


# ---------------------------------------------------------------------------------------------- the oracle's problem
def pose_problem(m, f, range_=2.0):
    """The Ceres problem Slam::SetupProblem would build if only frame f were free (rotation and translation), every
    point constant, no FrameDistance: the per-frame problem of tests/test_pose_gpu.py, restated."""
    from slamgpu.capi import ProblemArrays
    sel = usable_obs(m, f)
    pts, inv = np.unique(m.obs_point[sel], return_inverse=True)
    return ProblemArrays(
        k=m.k.copy(), q=m.q.reshape(-1, 4)[[f]].copy(), t=m.t.reshape(-1, 3)[[f]].copy(),
        frame_camera=m.frame_camera[[f]], frame_rot_free=[1], frame_trans_free=[1],
        X=m.X.reshape(-1, 4)[pts].copy(), point_free=np.zeros(len(pts), dtype=np.uint8),
        obs_pt=m.obs_pt.reshape(-1, 2)[sel].copy(), obs_frame=np.zeros(len(sel), dtype=np.int32), obs_point=inv,
        dist_frame=[], dist_prev=[], range_=range_, frame_map_index=[f], point_map_index=pts)


def oracle_pose(oracle_lib, m, f, q, t, options=None):
    """oracle.solve on frame f's problem started at (q, t): (summary, q, t)."""
    from slamgpu.capi import default_solver_options
    ms = m.copy()
    ms.q[4 * f:4 * f + 4], ms.t[3 * f:3 * f + 3] = q, t
    pa = pose_problem(ms, f)
    s = oracle_lib.solve(pa, options or default_solver_options())
    return s, pa.q[:4].copy(), pa.t[:3].copy()


def oracle_residuals(oracle_lib, m, f, q, t):
    ms = m.copy()
    ms.q[4 * f:4 * f + 4], ms.t[3 * f:3 * f + 3] = q, t
    r, _, nf = oracle_lib.evaluate(pose_problem(ms, f))
    assert nf == 0
    return r


# ---------------------------------------------------------------------------------------------- the tests' cases
SCENES = (("exact", 0.0), ("exact", 0.3), ("exact", 0.6), ("noisy", 0.3), ("noisy", 0.6))
COUNTS = (4, 5, 63, 64, 65, 255, 256, 257, 346)   # wave (64) and workgroup (256) boundaries; every record of frame 8
LONG_FRAME, LONG_COUNT = 2, 5588                  # make_scene(4, 6000, 11): past kPoseStage = 1024


def truncated(count: int, share: float, garbage: bool = True):
    """The exact C1 with frame 8 cut to its first `count` records, `share` outliers planted among them.  Returns
    (map, planted mask)."""
    m = base_scene("exact")
    sel = usable_obs(m, 8)
    assert len(sel) == 346
    m.obs_disabled[sel[count:]] = 1
    mask = plant_outliers(m, 8, share, 200 + count)
    if garbage:
        garbage_pose(m, [8])
    return m, mask


def long_scene(share: float, garbage: bool = True):
    """An exact scene whose frame 2 has 5588 records.  Returns (map, planted mask)."""
    if "long" not in _cache:
        from slamgpu.scene import make_scene
        _cache["long"] = make_scene(4, 6000, 11, noise=0.0, outlier_frac=0.0, perturb=False)
    m = _cache["long"].copy()
    assert len(usable_obs(m, LONG_FRAME)) == LONG_COUNT
    mask = plant_outliers(m, LONG_FRAME, share, 300)
    if garbage:
        garbage_pose(m, [LONG_FRAME])
    return m, mask


def all_cases():
    """Every (name, map with the true entry pose, frame, planted mask, exact?) the GPU tests check a mask on."""
    out = []
    for kind, share in SCENES:
        m, masks = scene(kind, share, garbage=False)
        out += [("%s %d%% frame %d" % (kind, round(100 * share), f), m, f, masks[f], kind == "exact") for f in FRAMES]
    for count in COUNTS:
        for share in (0.0, 0.3) if count >= 63 else (0.0,):
            m, mask = truncated(count, share, garbage=False)
            out.append(("frame 8 cut to %d, %d%%" % (count, round(100 * share)), m, 8, mask, True))
    for share in (0.0, 0.3):
        m, mask = long_scene(share, garbage=False)
        out.append(("long frame, %d%%" % round(100 * share), m, LONG_FRAME, mask, True))
    return out


# Records of the noisy scenes that are no planted outliers and still lie outside TAU at the oracle's optimum
# (0.5 px noise: 8 sigma), per (kind, share, frame); tests/test_localize_reference_bounds.py recounts them.
NOISY_INLIERS_OUTSIDE = 0
