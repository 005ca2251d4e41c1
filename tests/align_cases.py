"""Shared inputs and numpy references of the landmark-alignment tests (sg_slam_align_points, sg_map_apply_similarity).

Scenes.  Set A is the landmarks of the exact C1 scene (localize_cases.base_scene("exact")); set B is S_true applied to
A, appended to the map as new points; the correspondences are (a_i, b_i) in point order.  S_true is a rotation of 25
degrees about (1, 2, 3), the scale 1.3 and the translation (300, -200, 400); the "rigid" scenes use the scale 1.
  exact: no noise;
  noisy: Gaussian noise of TAU / 8 per coordinate on B (so that no true match leaves the TAU ball: 8 sigma);
  planted wrong matches: SHARE of the records get their B side moved by PLANT_MIN .. PLANT_MAX map units (at least
  10 TAU) in a random direction.
Hand-built scenes (collinear, thin, planar, mirrored, random) put both sides in as new points.

The references are restated here in numpy from the formulas of include/slamgpu.h and are never another path of the
library: the sampler (localize_cases.sample_np, the hash is the same), Horn's absolute orientation with the rotation
from np.linalg.svd and the gap from np.linalg.eigh of the 4x4 N (horn_np), the residual and the MSAC scorer
(score_np)."""
import numpy as np

import localize_cases as lc
from localize_cases import sample_np  # noqa: F401  (the sampler of sg_slam_localize_frames, used unchanged)
from slamgpu.scene import axis_angle, quat_from_matrix, quat_to_matrix

TAU = 10.0                  # threshold of every test, map units
SHARE = 0.3
PLANT_MIN, PLANT_MAX = 10.0 * TAU, 50.0 * TAU
NEAR = 1e-6                 # no record may lie this close to TAU at the reference estimate
H = 1024
SEED = 0
MARGIN = 100.0
MIN_GAP = 1e-6              # the default of sg_align_options
UNUSABLE = lc.UNUSABLE
MIN_W = 1e-9

R_TRUE = axis_angle(np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0) * np.radians(25.0))
T_TRUE = np.array([300.0, -200.0, 400.0])
SCALES = {"sim": 1.3, "rigid": 1.0}

COUNT_C1 = 484              # landmarks of C1 (all usable): recounted by tests/test_align_reference_bounds.py
COUNTS = (4, 5, 63, 64, 65, 255, 256, 257)   # wave (64) and workgroup (256) boundaries
LONG_COUNT = 1457           # make_scene(4, 1500, 11): past the 1024-record LDS stage

# The reference Horn's errors from one fixed well-spread sample of three records (spread_sample) on the exact scenes,
# worst over the exact cases of all_cases(): rotation (deg), translation (map units), |log scale| (never taken below one
# fp64 rounding, 2.2e-16: numpy often hits the scale exactly) and the worst residual over the true matches (map
# units).  tests/test_align_reference_bounds.py recomputes them and fails when a value is not an upper bound within a
# factor of 4.  The device gets MARGIN times them: another eigen-solver (Jacobi on the 4x4 instead of an SVD of the
# 3x3), another summation order and FMA contraction.
SPREAD_EXACT = {"rot_deg": 3.5e-14, "t": 4.5e-12, "log_scale": 2.3e-16, "resid": 8e-12}
# The all-inlier reference estimate's errors against the truth on the noisy cases (rotation deg, translation, |log
# scale|), worst over the cases of all_cases(): the same rule.
NOISY_POSE = {"rot_deg": 4e-3, "t": 0.2, "log_scale": 2e-5}
MIN_ALL_INLIER_SAMPLES = 300   # fewest all-inlier samples among the H hypotheses of seed SEED, over the planted cases

_cache = {}


# ---------------------------------------------------------------------------------------------- references
def horn_np(X, Y, fix_scale=False):
    """Horn's absolute orientation Y ~ s R X + t over the rows of X, Y: (s, R, t, gap).  R from the SVD of
    S = sum x' y'^T with the determinant fixed to +1; gap = (l3 - l2) / l3 of the 4x4 N."""
    X, Y = np.asarray(X, float), np.asarray(Y, float)
    xm, ym = X.mean(0), Y.mean(0)
    x, y = X - xm, Y - ym
    S = x.T @ y
    U, _, Vt = np.linalg.svd(S)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    N = np.array([
        [S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
        [0, S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
        [0, 0, -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
        [0, 0, 0, -S[0, 0] - S[1, 1] + S[2, 2]]])
    N = N + np.triu(N, 1).T
    w = np.linalg.eigvalsh(N)
    gap = (w[3] - w[2]) / w[3] if w[3] > 0 else 0.0
    s = 1.0 if fix_scale else float(np.sqrt((y * y).sum() / (x * x).sum()))
    return s, R, ym - s * R @ xm, float(gap)


def score_np(s, R, t, X, Y, tau=TAU):
    """Residuals e = |Y - (s R X + t)|, the inlier mask e^2 <= tau^2 and the MSAC cost sum min(e^2, tau^2)."""
    d = Y - (s * X @ R.T + t)
    e2 = (d * d).sum(1)
    inl = e2 <= tau * tau
    return np.sqrt(e2), inl, float(np.where(inl, e2, tau * tau).sum())


def rot_err_deg(R, Rt):
    c = (np.trace(R @ Rt.T) - 1.0) / 2.0
    # the angle from the skew part where the cosine has no resolution
    a = R @ Rt.T
    sn = 0.5 * np.linalg.norm([a[2, 1] - a[1, 2], a[0, 2] - a[2, 0], a[1, 0] - a[0, 1]])
    return float(np.degrees(np.arctan2(sn, c)))


def errors(s, R, t, kind="sim"):
    """(rotation deg, translation, |log scale|) of a transform against S_true of the scene kind."""
    return rot_err_deg(R, R_TRUE), float(np.linalg.norm(t - T_TRUE)), float(abs(np.log(s / SCALES[kind])))


def result_errors(res, kind="sim"):
    return errors(res["scale"], quat_to_matrix(res["q"]), res["t"], kind)


def within(err, bound, factor=1.0):
    return all(e <= factor * bound[k] for e, k in zip(err, ("rot_deg", "t", "log_scale")))


# ---------------------------------------------------------------------------------------------- scenes
def euclid(m, idx):
    X = m.X.reshape(-1, 4)[idx]
    return X[:, :3] / X[:, 3:4]


def append_points(m, E):
    """Appends the Euclidean points E (n, 3) to the map as unit-norm homogeneous points; returns their indices."""
    E = np.asarray(E, float).reshape(-1, 3)
    Xh = np.concatenate([E, np.ones((len(E), 1))], 1)
    Xh /= np.linalg.norm(Xh, axis=1, keepdims=True)
    first = m.num_points
    m.X = np.concatenate([m.X, Xh.reshape(-1)])
    m.point_flags = np.concatenate([m.point_flags, np.zeros(len(E), dtype=np.int32)])
    m.point_uncertainty = np.concatenate([m.point_uncertainty, np.ones(len(E))])
    if m.X_true is not None:
        m.X_true = np.concatenate([m.X_true, Xh.reshape(-1)])
    return np.arange(first, first + len(E), dtype=np.int32)


def apply_true(E, kind="sim"):
    return SCALES[kind] * E @ R_TRUE.T + T_TRUE


def records(m, corr):
    """(record mask over the correspondences, X (N, 3), Y (N, 3)): the record rule of include/slamgpu.h step 1."""
    corr = np.asarray(corr).reshape(-1, 2)
    X4 = m.X.reshape(-1, 4)
    ok = np.ones(len(corr), dtype=bool)
    for side in (0, 1):
        P = X4[corr[:, side]]
        ok &= (m.point_flags[corr[:, side]] & UNUSABLE) == 0
        ok &= np.isfinite(P).all(1)
        with np.errstate(invalid="ignore"):
            ok &= np.abs(P[:, 3]) >= MIN_W * np.linalg.norm(P, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ok, euclid(m, corr[ok, 0]), euclid(m, corr[ok, 1])


def plant(m, b_idx, share, seed):
    """Moves round(share * n) of the listed B points by PLANT_MIN .. PLANT_MAX in a random direction.  Returns the
    planted mask."""
    rng = np.random.default_rng(seed)
    n = len(b_idx)
    out = np.zeros(n, dtype=bool)
    out[rng.choice(n, size=int(round(share * n)), replace=False)] = True
    X4 = m.X.reshape(-1, 4)
    for j in np.flatnonzero(out):
        d = rng.normal(size=3)
        d *= rng.uniform(PLANT_MIN, PLANT_MAX) / np.linalg.norm(d)
        E = X4[b_idx[j], :3] / X4[b_idx[j], 3] + d
        X4[b_idx[j]] = np.append(E, 1.0) / np.linalg.norm(np.append(E, 1.0))
    return out


def _base(name):
    if name not in _cache:
        if name == "c1":
            _cache[name] = lc.base_scene("exact")
        else:
            from slamgpu.scene import make_scene
            _cache[name] = make_scene(4, 1500, 11, noise=0.0, outlier_frac=0.0, perturb=False)
    return _cache[name].copy()


def scene(noise="exact", share=0.0, kind="sim", count=None, base="c1", seed=1):
    """(map, corr (K, 2), planted mask): the first `count` landmarks of the base scene (all by default) as A, S_true
    of them as B with the noise and the planted wrong matches."""
    m = _base(base)
    a_idx = np.arange(m.num_points if count is None else count, dtype=np.int32)
    B = apply_true(euclid(m, a_idx), kind)
    rng = np.random.default_rng(1000 + seed)
    if noise == "noisy":
        B = B + rng.normal(0.0, TAU / 8.0, size=B.shape)
    else:
        assert noise == "exact"
    b_idx = append_points(m, B)
    planted = plant(m, b_idx, share, 2000 + seed + len(a_idx))
    return m, np.stack([a_idx, b_idx], 1), planted


def long_scene(share):
    return scene("exact", share, base="long", seed=7)


def hand_scene(A, B):
    """Both sides as new points of the exact C1 map: (map, corr)."""
    m = _base("c1")
    a_idx = append_points(m, A)
    b_idx = append_points(m, B)
    return m, np.stack([a_idx, b_idx], 1)


def _line_points(n, width, seed):
    """n points along a line through (500, -300, 3000), spread over about 2000 units, `width` off it."""
    rng = np.random.default_rng(seed)
    d = np.array([2.0, 1.0, -1.0]) / np.sqrt(6.0)
    u = np.array([1.0, -2.0, 0.0]) / np.sqrt(5.0)
    v = np.cross(d, u)
    a = rng.uniform(-1000.0, 1000.0, size=n)
    off = rng.uniform(-1.0, 1.0, size=(n, 2)) * width
    return np.array([500.0, -300.0, 3000.0]) + a[:, None] * d + off[:, :1] * u + off[:, 1:] * v


HAND_MIN_INLIERS_SHARE = 4  # the mirrored and random scenes ask for N / 4 inliers; numpy's best hypothesis has < N / 16
THIN_WIDTH = 0.02          # against a length of 2000: gap about 2 (w / L)^2, between 1e-12 and MIN_GAP / 100


def collinear_scene():
    A = _line_points(64, 0.0, 21)
    return hand_scene(A, apply_true(A))


def thin_scene():
    A = _line_points(64, THIN_WIDTH, 22)
    return hand_scene(A, apply_true(A))


def planar_scene():
    rng = np.random.default_rng(23)
    A = np.stack([rng.uniform(-1500, 1500, 64), rng.uniform(-1000, 1000, 64), np.full(64, 3000.0)], 1)
    A = A @ axis_angle(np.array([0.3, -0.2, 0.1])).T
    return hand_scene(A, apply_true(A))


def mirror_scene():
    """B is S_true of the mirror image of A: no proper rotation joins them."""
    m = _base("c1")
    A = euclid(m, np.arange(m.num_points))
    mid = A.mean(0)
    Am = A.copy()
    Am[:, 0] = 2.0 * mid[0] - Am[:, 0]
    return hand_scene(A, apply_true(Am))


def random_scene():
    m = _base("c1")
    A = euclid(m, np.arange(m.num_points))
    rng = np.random.default_rng(24)
    return hand_scene(A, rng.uniform(A.min(0), A.max(0), size=A.shape))


def spread_sample(X):
    """The fixed, well-spread sample of the reference bound: the records of smallest and largest x, and the one
    farthest from the line through them."""
    i0, i1 = int(np.argmin(X[:, 0])), int(np.argmax(X[:, 0]))
    d = (X[i1] - X[i0]) / np.linalg.norm(X[i1] - X[i0])
    r = X - X[i0]
    i2 = int(np.argmax(np.linalg.norm(r - (r @ d)[:, None] * d, axis=1)))
    assert len({i0, i1, i2}) == 3
    return [i0, i1, i2]


# ---------------------------------------------------------------------------------------------- the tests' cases
def count_cases():
    return [(c, s) for c in COUNTS for s in ((0.0, SHARE) if c >= 63 else (0.0,))]


def all_cases():
    """Every (name, map, corr, planted, noise, kind) the GPU tests check a mask on."""
    out = []
    for noise in ("exact", "noisy"):
        for share in (0.0, SHARE):
            for kind in ("sim", "rigid"):
                m, corr, planted = scene(noise, share, kind)
                out.append(("%s %s %d%%" % (noise, kind, round(100 * share)), m, corr, planted, noise, kind))
    for count, share in count_cases():
        m, corr, planted = scene("exact", share, count=count)
        out.append(("cut to %d, %d%%" % (count, round(100 * share)), m, corr, planted, "exact", "sim"))
    for share in (0.0, SHARE):
        m, corr, planted = long_scene(share)
        out.append(("long group, %d%%" % round(100 * share), m, corr, planted, "exact", "sim"))
    return out


def numpy_apply(m, s, R, t, frames, points):
    """sg_map_apply_similarity restated: a transformed copy of the map."""
    o = m.copy()
    X4 = o.X.reshape(-1, 4)
    for p in points:
        X4[p, :3] = s * R @ X4[p, :3] + t * X4[p, 3]
    for f in frames:
        o.t[3 * f:3 * f + 3] = s * R @ m.t[3 * f:3 * f + 3] + t
        o.q[4 * f:4 * f + 4] = quat_from_matrix(quat_to_matrix(m.q[4 * f:4 * f + 4]) @ R.T)
    return o
