"""Shared inputs and numpy references of the relative-pose tests (csrc/relpose_math.h and sg_slam_relative_poses).

Scenes come from make_config("C1", outlier_frac=0, perturb=False), as localize_cases.base_scene does:
  exact: noise=0, so every pixel is the projection of its point;
  noisy: the stock 0.5 px pixel noise; the outliers are the planted ones only.
plant_outliers replaces the pixel in frame b of a share of a pair's records by a pixel uniform in the image, at least
MIN_OUTLIER_PX from the true epipolar line in b and with its own epipolar line in a at least MIN_OUTLIER_PX from the
pixel in a, so the expected inlier mask is known (a pixel merely far from the true point lies within the threshold of
the epipolar line about 1 % of the time).

The references are restated here in numpy and are never another path of the library: the sampler (sample_np, the hash
of sg_slam_localize_frames extended to eight indices), the normalised 8-point by np.linalg.eigh and np.linalg.svd
(eight_point_np), the Sampson score (sampson_np, score_np) and the decomposition with np.linalg.lstsq (decompose_np)."""
import numpy as np

from slamgpu.scene import HEIGHT, WIDTH, make_config, quat_to_matrix

TAU = 2.0                   # threshold_px of every test
MIN_OUTLIER_PX = 20.0       # planted outliers: distance from both epipolar lines
NEAR = 1e-6                 # no record of a test case may lie this close to TAU at the reference estimate
PAIRS = ((4, 5), (3, 8), (1, 2), (2, 8))   # the C1 pairs the tests solve
COUNTS_C1 = {(4, 5): 211, (3, 8): 101, (1, 2): 97, (2, 8): 73, (0, 9): 14}   # records, recounted by the bounds test
SEED = 0                    # the sampler seed the sample counts below are for
H = 1024                    # the hypothesis count they are for
SHARE = 0.3                 # the share of planted outliers

# On the exact scenes, the reference 8-point from the fixed well-spread sample of spread_sample(): the largest
# rotation error (deg), translation-direction error (deg) and Sampson error (px) over PAIRS.  Recomputed by
# tests/test_relpose_reference_bounds.py, which fails when a value is not an upper bound within a factor of 4.  The
# device gets MARGIN times them: another eigen-solver (an LDL^T with inverse iterations instead of LAPACK's eigh and
# svd), another summation order and FMA contraction, as the localization tests argue.
SPREAD_EXACT = {"rot_deg": 2e-8, "dir_deg": 2e-7, "sampson_px": 2e-7}
MARGIN = 100.0

# Rotation and direction error (deg) of the reference all-inlier 8-point on the noisy scenes, the largest over the
# shares 0 and SHARE, per pair; recomputed by the bounds test (upper bound within a factor of 4).  The device with
# refine is held to twice these: the same estimator on the same inliers.
NOISY_POSE = {(4, 5): (0.1, 2.0), (3, 8): (0.12, 0.3), (1, 2): (0.12, 0.6), (2, 8): (0.12, 0.5)}
# Records of the noisy scenes that are not planted and still lie outside TAU at that estimate (recounted).
NOISY_INLIERS_OUTSIDE = 0
# The fewest all-inlier samples among the H hypotheses of seed SEED over the cases with planted outliers (recounted;
# a RANSAC test needs at least 8).
MIN_ALL_INLIER_SAMPLES = 40

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


def pair_key(a: int, b: int) -> int:
    return a * 65536 + b


def sample_np(seed: int, key: int, h: int, n: int) -> tuple:
    """Hypothesis h of the pair with key a * 65536 + b over n records: eight distinct indices in draw order."""
    base = mix(mix(mix(seed) + key) + h)
    taken, out = [], []
    for j in range(8):
        r = mix(base ^ ((0x9E3779B9 * (j + 1)) & _M32))
        i = (r * (n - j)) >> 32
        for p in sorted(taken):
            if i >= p:
                i += 1
        taken.append(i)
        out.append(i)
    return tuple(out)


# ---------------------------------------------------------------------------------------------- geometry
def undistort_np(k, pt):
    """Pixels (n, 2) -> plane coordinates (n, 2): the radial distortion inverted by Newton on the radius."""
    xd, yd = (pt[:, 0] - k[5]) / k[3], (pt[:, 1] - k[6]) / k[4]
    rd = np.hypot(xd, yd)
    r = rd.copy()
    for _ in range(20):
        r2 = r * r
        fr = r * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) - rd
        df = 1 + r2 * (3 * k[0] + r2 * (5 * k[1] + r2 * 7 * k[2]))
        r = r - fr / df
    s = np.where(rd > 0, r / np.where(rd > 0, rd, 1.0), 0.0)
    return np.stack([xd * s, yd * s], 1)


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def hartley(x):
    """(n, 2) -> (normalised homogeneous (n, 3), T): centroid to the origin, rms distance to sqrt 2."""
    c = x.mean(0)
    s = np.sqrt(2.0) / np.sqrt(((x - c) ** 2).sum(1).mean())
    T = np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])
    return np.concatenate([s * (x - c), np.ones((len(x), 1))], 1), T


def to_essential(E):
    """The nearest matrix with singular values (1, 1, 0)."""
    U, _, Vt = np.linalg.svd(E)
    return U @ np.diag([1.0, 1.0, 0.0]) @ Vt


def eight_point_np(xa, xb):
    """Normalised 8-point on plane coordinates (n >= 8): (E with singular values (1, 1, 0), the null vector of the
    normalised moment matrix, its eigenvalues ascending).  x_b^T E x_a = 0."""
    ha, Ta = hartley(xa)
    hb, Tb = hartley(xb)
    A = np.einsum("ni,nj->nij", hb, ha).reshape(-1, 9)
    w, V = np.linalg.eigh(A.T @ A)
    e = V[:, 0]
    return to_essential(Tb.T @ e.reshape(3, 3) @ Ta), e, w


def sampson_np(E, xa, xb, ka, kb):
    """Squared Sampson distance in ideal pixels: F = K_b^-T E K_a^-1 applied to (fx x + cx, fy y + cy)."""
    ha = np.concatenate([xa, np.ones((len(xa), 1))], 1)
    hb = np.concatenate([xb, np.ones((len(xb), 1))], 1)
    lb = ha @ E.T          # E x_a: the line in b
    la = hb @ E            # E^T x_b: the line in a
    num = (hb * lb).sum(1) ** 2
    den = (lb[:, 0] / kb[3]) ** 2 + (lb[:, 1] / kb[4]) ** 2 + (la[:, 0] / ka[3]) ** 2 + (la[:, 1] / ka[4]) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / den


def score_np(E, xa, xb, ka, kb, tau=TAU):
    """(Sampson errors e in px, inlier mask e^2 <= tau^2, MSAC cost sum min(e^2, tau^2))."""
    e2 = sampson_np(E, xa, xb, ka, kb)
    e2 = np.where(np.isfinite(e2), e2, np.inf)
    inl = e2 <= tau * tau
    return np.sqrt(e2), inl, float(np.where(inl, e2, tau * tau).sum())


def decompose_np(E, xa, xb, inl):
    """The four (R, t) of E = [t]x R (p_b = R p_a + t), each tested on the inliers by the least-squares depths of
    d_b f_b = d_a R f_a + t (np.linalg.lstsq): (R, t, in-front mask, parallax in rad) of the one with the most records
    in front of both cameras, ties to the earlier of (R1, +u3), (R1, -u3), (R2, +u3), (R2, -u3)."""
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U[:, 2] = -U[:, 2]
    if np.linalg.det(Vt) < 0:
        Vt[2, :] = -Vt[2, :]
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    fa = np.concatenate([xa, np.ones((len(xa), 1))], 1)
    fb = np.concatenate([xb, np.ones((len(xb), 1))], 1)
    best = None
    for R in (U @ W @ Vt, U @ W.T @ Vt):
        for t in (U[:, 2], -U[:, 2]):
            g = fa @ R.T
            front = np.zeros(len(xa), dtype=bool)
            for i in np.flatnonzero(inl):
                d = np.linalg.lstsq(np.stack([g[i], -fb[i]], 1), -t, rcond=None)[0]
                front[i] = d[0] > 0 and d[1] > 0
            if best is None or front.sum() > best[2].sum():
                par = np.arctan2(np.linalg.norm(np.cross(g, fb), axis=1), (g * fb).sum(1))
                best = (R, t, front, par)
    return best


def rel_from_cv(R, t):
    """(R, t) of p_b = R p_a + t -> the map's convention p_b = R (p_a - t_rel): t_rel = -R^T t, unit."""
    t_rel = -R.T @ t
    return R, t_rel / np.linalg.norm(t_rel)


def true_rel(m, a, b):
    """(R_rel, unit t_rel, baseline) of frames a, b from the ground truth: p_b = R_rel (p_a - baseline t_rel)."""
    Ra, Rb = quat_to_matrix(m.q_true[4 * a:4 * a + 4]), quat_to_matrix(m.q_true[4 * b:4 * b + 4])
    d = Ra @ (m.t_true[3 * b:3 * b + 3] - m.t_true[3 * a:3 * a + 3])
    base = float(np.linalg.norm(d))
    return Rb @ Ra.T, d / base, base


def true_essential(m, a, b):
    R, t_rel, _ = true_rel(m, a, b)
    return to_essential(skew(-R @ t_rel) @ R)


def rot_err_deg(R, R_true):
    c = 0.5 * (np.trace(R @ R_true.T) - 1.0)
    s = 0.5 * np.linalg.norm([(R @ R_true.T)[2, 1] - (R @ R_true.T)[1, 2], (R @ R_true.T)[0, 2] - (R @ R_true.T)[2, 0],
                              (R @ R_true.T)[1, 0] - (R @ R_true.T)[0, 1]])
    return float(np.degrees(np.arctan2(s, c)))


def dir_err_deg(t, t_true):
    return float(np.degrees(np.arctan2(np.linalg.norm(np.cross(t, t_true)), np.dot(t, t_true))))


# ---------------------------------------------------------------------------------------------- records
def pair_obs(m, a, b):
    """(observation indices in a, in b) of the pair's records: points with an enabled observation in both frames, in
    the map order of a's observations, the first enabled observation of the point in each frame."""
    first_b, seen, oa, ob = {}, set(), [], []
    for o in np.flatnonzero((m.obs_frame == b) & (m.obs_disabled == 0)):
        first_b.setdefault(int(m.obs_point[o]), int(o))
    for o in np.flatnonzero((m.obs_frame == a) & (m.obs_disabled == 0)):
        p = int(m.obs_point[o])
        if p in seen:
            continue
        seen.add(p)
        if p in first_b:
            oa.append(int(o))
            ob.append(first_b[p])
    return np.array(oa, dtype=np.int64), np.array(ob, dtype=np.int64)


def pair_records(m, a, b):
    """(obs in a, obs in b, plane coordinates in a (n, 2), in b (n, 2), intrinsics of a, of b)."""
    oa, ob = pair_obs(m, a, b)
    ka = m.k[7 * m.frame_camera[a]:7 * m.frame_camera[a] + 7]
    kb = m.k[7 * m.frame_camera[b]:7 * m.frame_camera[b] + 7]
    pts = m.obs_pt.reshape(-1, 2)
    return oa, ob, undistort_np(ka, pts[oa]), undistort_np(kb, pts[ob]), ka, kb


# ---------------------------------------------------------------------------------------------- scenes
def base_scene(kind: str):
    """'exact' or 'noisy' C1, poses and points the truth.  A fresh copy per call."""
    if kind not in _cache:
        kw = dict(outlier_frac=0.0, perturb=False)
        if kind == "exact":
            kw["noise"] = 0.0
        else:
            assert kind == "noisy"
        _cache[kind] = make_config("C1", **kw)
    return _cache[kind].copy()


def _line_dist_px(l, u):
    return abs(l[0] * u[0] + l[1] * u[1] + l[2]) / np.hypot(l[0], l[1])


def plant_outliers(m, a, b, share: float, seed: int):
    """Replaces the pixel in b of round(share * N) of the pair's records (chosen by the seeded generator) by a pixel
    uniform in the image, at least MIN_OUTLIER_PX from the true epipolar line in b and whose own epipolar line in a is
    at least MIN_OUTLIER_PX from the pixel in a.  Returns the planted mask over the pair's records."""
    oa, ob, _, _, ka, kb = pair_records(m, a, b)
    rng = np.random.default_rng(seed)
    n = len(oa)
    Ka =np.array([[ka[3], 0, ka[5]], [0, ka[4], ka[6]], [0, 0, 1.0]])
    Kb = np.array([[kb[3], 0, kb[5]], [0, kb[4], kb[6]], [0, 0, 1.0]])
    assert not ka[:3].any() and not kb[:3].any()   # the C1 cameras have no distortion: pixels are ideal pixels
    F = np.linalg.inv(Kb).T @ true_essential(m, a, b) @ np.linalg.inv(Ka)
    pts = m.obs_pt.reshape(-1, 2)
    # every epipolar line in a passes through the epipole, so a record whose pixel in a is near it cannot be planted
    # under the rule: those records are never chosen (with forward motion the epipole is inside the image)
    ep = np.linalg.svd(F)[2][2]
    far = np.ones(n, dtype=bool)
    if abs(ep[2]) > 1e-12 * np.abs(ep).max():
        far = np.hypot(*(pts[oa] - ep[:2] / ep[2]).T) >= 3 * MIN_OUTLIER_PX
    out = np.zeros(n, dtype=bool)
    out[rng.choice(np.flatnonzero(far), size=int(round(share * n)), replace=False)] = True
    for j in np.flatnonzero(out):
        ua = np.array([*pts[oa[j]], 1.0])
        while True:
            p = rng.uniform((0.0, 0.0), (WIDTH, HEIGHT))
            ub = np.array([*p, 1.0])
            if _line_dist_px(F @ ua, ub) >= MIN_OUTLIER_PX and _line_dist_px(F.T @ ub, ua) >= MIN_OUTLIER_PX:
                break
        pts[ob[j]] = p
    return out


def garbage_poses(m, frames):
    """The entry pose of the listed frames becomes garbage: looking the other way, 100 m off."""
    for f in frames:
        m.q[4 * f:4 * f + 4] = (0.5, -0.5, 0.5, 0.5)
        m.t[3 * f:3 * f + 3] = (1e5, -2e5, 3e5)


def scene(kind: str, share: float, pair):
    """The scene `kind` with `share` outliers planted in the one pair (seed 100 + 16 a + b).  Returns (map, planted
    mask over the pair's records)."""
    m = base_scene(kind)
    a, b = pair
    n = len(pair_obs(m, a, b)[0])
    mask = plant_outliers(m, a, b, share, 100 + 16 * a + b) if share > 0 else np.zeros(n, dtype=bool)
    return m, mask


# One call may not list a frame as b twice, and PAIRS has frame 8 as b of two pairs: the batch takes (3, 8) reversed.
BATCH_PAIRS = ((4, 5), (2, 8), (1, 2), (8, 3))


def batch_scene():
    """The exact scene with SHARE outliers planted in every pair of PAIRS, one after the other.  Frame 8 is the b of
    two pairs, so the masks are not known: for comparisons of bits only."""
    m = base_scene("exact")
    for a, b in PAIRS:
        plant_outliers(m, a, b, SHARE, 100 + 16 * a + b)
    return m


def truncated(count: int, share: float):
    """The exact C1 with pair (4, 5) cut to its first `count` records (the later observations of frame 4 disabled),
    `share` outliers planted among them.  Returns (map, planted mask)."""
    m = base_scene("exact")
    oa, _ = pair_obs(m, 4, 5)
    assert len(oa) == COUNTS_C1[(4, 5)]
    m.obs_disabled[oa[count:]] = 1
    mask = plant_outliers(m, 4, 5, share, 200 + count) if share > 0 else np.zeros(count, dtype=bool)
    return m, mask


LONG_PAIR, LONG_COUNT = (2, 3), 5312   # make_scene(4, 6000, 11): past the 1024-record LDS stage


def long_scene(share: float):
    """An exact scene whose pair LONG_PAIR has LONG_COUNT > 1024 records.  Returns (map, planted mask)."""
    if "long" not in _cache:
        from slamgpu.scene import make_scene
        _cache["long"] = make_scene(4, 6000, 11, noise=0.0, outlier_frac=0.0, perturb=False)
    m = _cache["long"].copy()
    n = len(pair_obs(m, *LONG_PAIR)[0])
    assert n == LONG_COUNT, n
    mask = plant_outliers(m, *LONG_PAIR, share, 300) if share > 0 else np.zeros(n, dtype=bool)
    return m, mask


# ---------------------------------------------------------------------------------------------- hand-built scenes
PARALLAX_GATE = np.radians(2.0)       # min_parallax of the count test on pair (4, 5): inside its 0 .. 8 degree spread
NEAR_ROTATION_MM = 5.0                # baseline of the almost-pure rotation: 5 mm against depths of 1000 mm and more
NEAR_ROTATION_GATE = np.radians(1.0)  # min_parallax of that test
# The largest parallax (deg) of a record of near_rotation_scene(), recomputed by the bounds test (upper bound within a
# factor of 4): atan(5 / 1000) = 0.29 deg is the limit, far below the 1 degree gate.
NEAR_ROTATION_MAX_PARALLAX_DEG = 0.3
PARALLAX_NEAR = 1e-9                  # no record's true parallax may lie this close (rad) to a gate


def _project_into(m, f, Xw, R, c):
    """Pixels of the Euclidean world points Xw in a camera with frame f's intrinsics, rotation R and centre c."""
    k = m.k[7 * m.frame_camera[f]:7 * m.frame_camera[f] + 7]
    assert not k[:3].any()
    p = (Xw - c) @ R.T
    assert (p[:, 2] > 1.0).all()
    return np.stack([k[3] * p[:, 0] / p[:, 2] + k[5], k[4] * p[:, 1] / p[:, 2] + k[6]], 1)


def true_parallax(m, a, b):
    """Per record of the pair, the angle (rad) between R_rel f_a and f_b at the ground truth."""
    _, _, xa, xb, _, _ = pair_records(m, a, b)
    R = true_rel(m, a, b)[0]
    g = np.concatenate([xa, np.ones((len(xa), 1))], 1) @ R.T
    fb = np.concatenate([xb, np.ones((len(xb), 1))], 1)
    return np.arctan2(np.linalg.norm(np.cross(g, fb), axis=1), (g * fb).sum(1))


def near_rotation_scene():
    """The exact C1 with frame 5 moved to NEAR_ROTATION_MM from frame 4's centre along frame 4's x axis, its rotation
    kept, and its observations of the pair's points re-projected exactly: an almost pure rotation, every parallax
    below NEAR_ROTATION_MAX_PARALLAX_DEG.  The ground truth of frame 5 is updated, so true_rel holds."""
    m = base_scene("exact")
    oa, ob = pair_obs(m, 4, 5)
    Ra, Rb = quat_to_matrix(m.q_true[16:20]), quat_to_matrix(m.q_true[20:24])
    c = m.t_true[12:15] + Ra.T @ np.array([NEAR_ROTATION_MM, 0.0, 0.0])
    X = m.X_true.reshape(-1, 4)[m.obs_point[ob]]
    m.obs_pt.reshape(-1, 2)[ob] = _project_into(m, 5, X[:, :3] / X[:, 3:4], Rb, c)
    m.t_true[15:18] = c
    m.t[15:18] = c
    return m


def planar_scene():
    """The exact C1 with the points of pair (4, 5) moved onto one plane (z = 3000 + 0.2 x - 0.1 y in frame 4's
    coordinates, along frame 4's rays) and both frames' observations of them re-projected exactly: the configuration
    on which the 8-point is degenerate."""
    m = base_scene("exact")
    oa, ob = pair_obs(m, 4, 5)
    _, _, xa, _, _, _ = pair_records(m, 4, 5)
    Ra, Rb = quat_to_matrix(m.q_true[16:20]), quat_to_matrix(m.q_true[20:24])
    z = 3000.0 / (1.0 - 0.2 * xa[:, 0] + 0.1 * xa[:, 1])
    Xw = (np.concatenate([xa, np.ones((len(xa), 1))], 1) * z[:, None]) @ Ra + m.t_true[12:15]
    m.obs_pt.reshape(-1, 2)[ob] = _project_into(m, 5, Xw, Rb, m.t_true[15:18])
    return m


ANCHORS = np.array([(60.0, 50.0), (320.0, 40.0), (580.0, 50.0), (70.0, 240.0), (570.0, 240.0), (60.0, 430.0),
                    (320.0, 440.0), (580.0, 430.0)])


def spread_sample(pt_a):
    """The fixed, well-spread sample of the reference bound: the records whose pixel in a is nearest to eight image
    anchors (the corners, the edge centres), each taken once."""
    idx = []
    for anchor in ANCHORS:
        d = ((pt_a - anchor) ** 2).sum(1)
        d[idx] = np.inf
        idx.append(int(np.argmin(d)))
    assert len(set(idx)) == 8
    return idx


# ---------------------------------------------------------------------------------------------- the tests' cases
COUNTS = (8, 9, 63, 64, 65, 211)   # pair (4, 5) cut to these; SHARE only from 63 up


def count_cases():
    return [(c, s) for c in COUNTS for s in ((0.0, SHARE) if c >= 63 else (0.0,))]


def all_cases():
    """Every (name, map, pair, planted mask, exact?) a mask is checked on."""
    out = []
    for kind in ("exact", "noisy"):
        for share in (0.0, SHARE):
            for p in PAIRS:
                m, mask = scene(kind, share, p)
                out.append(("%s %d%% pair %s" % (kind, round(100 * share), p), m, p, mask, kind == "exact"))
    for count, share in count_cases():
        m, mask = truncated(count, share)
        out.append(("pair (4, 5) cut to %d, %d%%" % (count, round(100 * share)), m, (4, 5), mask, True))
    for share in (0.0, SHARE):
        m, mask = long_scene(share)
        out.append(("long pair, %d%%" % round(100 * share), m, LONG_PAIR, mask, True))
    return out
