"""Scenes and the numpy reference of sg_slam_match_by_projection (include/slamgpu.h).  Test material only: nothing here
is a path of the library.

Scenes: make_config("C1", noise=0, outlier_frac=0, perturb=False), and the long case with num_points=6000.  Camera 1's
intrinsics are overwritten with a distorted set of another focal length (the stock cameras are identical, which would
hide a frame_camera indexing error), and the observation pixels are recomputed for it.  Every landmark gets a random
256-bit descriptor; a frame's keypoints are its observation pixels with the landmark's descriptor after
Binomial(256, 0.03) bit flips, plus distractor keypoints with fresh random descriptors at random pixels, all shuffled.
Every second observation of the map is disabled, so that skip_observed has both kinds to tell apart.

The planted scene holds hand-placed points and keypoints in one frame for every rule of the contract (planted()).

The reference (reference()) is the contract written plainly: projection, culls, windows, best, second, counts,
acceptance, uniqueness.  Its `off` argument switches single rules off, for the tests that show each planted case
bites."""
import functools
from types import SimpleNamespace

import numpy as np

from slamgpu.scene import HEIGHT, WIDTH, make_config, quat_to_matrix

RADIUS = 12.0
CHUNK = 64           # kMatchChunk of csrc/match_plan.h
SLICE = 512          # kMatchSlice of csrc/match_plan.h (held equal by test_match_plan.py)
K_DISTORTED = np.array([-0.05, 0.01, -0.002, 380.0, -380.0, 330.0, 230.0])
FLIP_P = 0.03
NEAR = 1e-6          # px: no distance this close to the radius, no projection this close to a border
NEAR_Z = 1e-9        # relative: no p.z this close to the 0.001 W refusal line


# ------------------------------------------------------------------------------------------------ the reference
def popcount(a):
    """Set bits per row of a uint64 array (..., 4)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape[:-1] + (32,)), axis=-1).sum(-1).astype(np.int64)


def project(q, t, k, X):
    """Project of csrc/project_math.h on homogeneous rows X (n, 4), in its order of operations: pixels (n, 2), the
    accepted mask (not behind the camera) and p.z - 0.001 W."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        v = X[:, :3] - np.asarray(t)[None, :] * X[:, 3:4]
        c = np.stack([q[1] * v[:, 2] - q[2] * v[:, 1], q[2] * v[:, 0] - q[0] * v[:, 2],
                      q[0] * v[:, 1] - q[1] * v[:, 0]], 1)
        c = c + c
        p = np.stack([(v[:, 0] + q[3] * c[:, 0]) + (q[1] * c[:, 2] - q[2] * c[:, 1]),
                      (v[:, 1] + q[3] * c[:, 1]) + (q[2] * c[:, 0] - q[0] * c[:, 2]),
                      (v[:, 2] + q[3] * c[:, 2]) + (q[0] * c[:, 1] - q[1] * c[:, 0])], 1)
        ok = ~(p[:, 2] < 0.001 * X[:, 3])
        xp, yp = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
        r2 = xp * xp + yp * yp
        d = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
        uv = np.stack([xp * d * k[3] + k[5], yp * d * k[4] + k[6]], 1)
    return uv, ok, p[:, 2] - 0.001 * X[:, 3]


def reference(case, off=()):
    """The contract on one case, per listed frame: a dict of match, best_point, best_dist, second_dist, num_candidates
    (int32 per keypoint), the four counts of sg_match_result, and the input margins (radius_gap, border_gap, z_gap:
    how close the case comes to a decision that rounding could turn).  off: rules switched off, any of "exclusion",
    "bounds", "tie", "ratio", "unique"."""
    m, o = case.m, case.options
    pts = np.asarray(case.points, dtype=np.int64)
    pd = np.asarray(case.point_desc, dtype=np.uint64).reshape(-1, 4)
    X4 = m.X.reshape(-1, 4)[pts] if len(pts) else np.zeros((0, 4))
    bounded = o["width"] > 0 and "bounds" not in off
    out = []
    for f, (xy, kd) in zip(case.frames, case.keypoints):
        xy, kd = np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(kd, dtype=np.uint64).reshape(-1, 4)
        cam = m.frame_camera[f]
        uv, ok, zgap = project(m.q[4 * f:4 * f + 4], m.t[3 * f:3 * f + 3], m.k[7 * cam:7 * cam + 7], X4)
        with np.errstate(invalid="ignore"):
            z_gap = np.nanmin(np.abs(zgap) / np.maximum(np.abs(0.001 * X4[:, 3]), 1e-300), initial=np.inf)
            cand = ok & np.isfinite(uv).all(1)
            border_gap = np.inf
            if o["width"] > 0 and cand.any():
                c = uv[cand]
                border_gap = min(np.abs(c[:, 0]).min(), np.abs(c[:, 0] - o["width"]).min(), np.abs(c[:, 1]).min(),
                                 np.abs(c[:, 1] - o["height"]).min())
            if bounded:
                cand &= (uv[:, 0] >= 0) & (uv[:, 0] < o["width"]) & (uv[:, 1] >= 0) & (uv[:, 1] < o["height"])
        if o["skip_observed"] and "exclusion" not in off:
            seen = m.obs_point[(m.obs_frame == f) & (m.obs_disabled == 0)]
            cand &= ~np.isin(pts, seen)
        pos = np.flatnonzero(cand)          # positions in points[], ascending
        cu, cd = uv[pos], pd[pos]
        K = len(xy)
        bp, bd, sd = (np.full(K, -1, dtype=np.int32) for _ in range(3))
        nc = np.zeros(K, dtype=np.int32)
        radius_gap = np.inf
        r2 = o["radius_px"] * o["radius_px"]
        for i in range(K):
            if not np.isfinite(xy[i]).all() or len(pos) == 0:
                continue
            du, dv = cu[:, 0] - xy[i, 0], cu[:, 1] - xy[i, 1]
            d2 = du * du + dv * dv
            radius_gap = min(radius_gap, np.abs(np.sqrt(d2) - o["radius_px"]).min())
            w = np.flatnonzero(d2 <= r2)
            nc[i] = len(w)
            if len(w) == 0:
                continue
            h = popcount(cd[w] ^ kd[i][None, :])
            order = np.lexsort((-pos[w] if "tie" in off else pos[w], h))
            bp[i], bd[i] = pts[pos[w[order[0]]]], h[order[0]]
            if len(w) > 1:
                sd[i] = h[order[1]]
        accept = (bp >= 0) & (bd <= o["max_dist"])
        if "ratio" not in off:
            accept &= (sd < 0) | (100 * bd.astype(np.int64) <= o["ratio_percent"] * sd.astype(np.int64))
        match = np.where(accept, bp, -1).astype(np.int32)
        if "unique" not in off:
            for p in np.unique(match[match >= 0]):
                who = np.flatnonzero(match == p)
                keep = who[np.lexsort((who, bd[who]))[0]]
                match[who[who != keep]] = -1
        out.append(dict(match=match, best_point=bp, best_dist=bd, second_dist=sd, num_candidates=nc,
                        num_keypoints=K, num_projected=len(pos), num_with_candidates=int((nc > 0).sum()),
                        num_matched=int((match >= 0).sum()), radius_gap=radius_gap, border_gap=border_gap,
                        z_gap=z_gap))
    return out


# ------------------------------------------------------------------------------------------------ generated scenes
def _flip(rng, desc, p=FLIP_P):
    flips = rng.random((len(desc), 256)) < p
    return desc ^ np.packbits(flips, axis=1, bitorder="little").view(np.uint64).reshape(len(desc), 4)


def _random_desc(rng, n):
    return rng.integers(0, 2 ** 64, size=(n, 4), dtype=np.uint64, endpoint=False)


@functools.lru_cache(maxsize=None)
def scene(long=False):
    """(map, descriptors of all its points)."""
    kw = dict(noise=0, outlier_frac=0, perturb=False)
    if long:
        kw["num_points"] = 6000
    m = make_config("C1", **kw)
    m.k[7:14] = K_DISTORTED
    X4 = m.X.reshape(-1, 4)
    for f in range(m.num_frames):
        sel = np.flatnonzero(m.obs_frame == f)
        cam = m.frame_camera[f]
        uv, ok, _ = project(m.q[4 * f:4 * f + 4], m.t[3 * f:3 * f + 3], m.k[7 * cam:7 * cam + 7], X4[m.obs_point[sel]])
        assert ok.all()
        m.obs_pt.reshape(-1, 2)[sel] = uv
    m.obs_disabled[1::2] = 1
    rng = np.random.default_rng(77 if long else 76)
    return m, _random_desc(rng, m.num_points)


def frame_keypoints(m, desc, f, seed, distract=0.25):
    """The frame's observation pixels with flipped descriptors, and distractors, shuffled."""
    rng = np.random.default_rng(seed)
    sel = np.flatnonzero(m.obs_frame == f)
    xy = m.obs_pt.reshape(-1, 2)[sel].copy()
    kd = _flip(rng, desc[m.obs_point[sel]])
    nd = int(distract * len(sel)) + 3
    xy = np.concatenate([xy, np.stack([rng.uniform(0, WIDTH, nd), rng.uniform(0, HEIGHT, nd)], 1)])
    kd = np.concatenate([kd, _random_desc(rng, nd)])
    order = rng.permutation(len(xy))
    return xy[order], kd[order]


def options(**kw):
    o = dict(radius_px=RADIUS, width=0, height=0, max_dist=64, ratio_percent=80, skip_observed=1)
    o.update(kw)
    return o


def generated(long, frames, **opt):
    m, desc = scene(long)
    kps = [frame_keypoints(m, desc, f, 1000 + f) for f in frames]
    rng = np.random.default_rng(5)
    points = rng.permutation(m.num_points).astype(np.int32)     # positions are not map indices
    return SimpleNamespace(m=m, frames=list(frames), keypoints=kps, points=points, point_desc=desc[points],
                           options=options(**opt))


# ------------------------------------------------------------------------------------------------ the planted scene
PLANT_FRAME = 4      # a frame of camera 1, the distorted one


def _world(m, f, xn, yn, depth):
    """The homogeneous world point at camera coordinates depth * (xn, yn, 1) of frame f (W = 1, not normalised)."""
    R = quat_to_matrix(m.q[4 * f:4 * f + 4])
    return np.concatenate([R.T @ (depth * np.array([xn, yn, 1.0])) + m.t[3 * f:3 * f + 3], [1.0]])


@functools.lru_cache(maxsize=None)
def _planted_base():
    """The C1 scene with the planted points appended and their descriptors; the planted keypoints of PLANT_FRAME."""
    m0, _ = scene(False)
    m = m0.copy()
    rng = np.random.default_rng(99)
    f = PLANT_FRAME
    assert m.frame_camera[f] == 1
    names = ["behind", "nan", "left", "single", "tie_hi", "tie_lo", "seen", "unseen", "shared", "shared_eq", "alike_a",
             "alike_b", "far"]
    spots = dict(behind=(0.05, 0.05, -2000.0), nan=(0.0, 0.0, 1.0), left=(-0.93, 0.1, 2500.0),
                 single=(-0.4, -0.3, 1500.0), tie_hi=(0.30, 0.30, 3000.0), tie_lo=(0.31, 0.30, 3000.0),
                 seen=(-0.30, 0.30, 2000.0), unseen=(-0.29, 0.31, 2200.0), shared=(0.5, -0.4, 4000.0),
                 shared_eq=(0.1, -0.45, 4000.0), alike_a=(0.6, 0.2, 1800.0), alike_b=(0.61, 0.21, 1800.0),
                 far=(0.0, 0.5, 5000.0))
    P0 = m.num_points
    idx = {nm: P0 + i for i, nm in enumerate(names)}
    Xn = np.stack([_world(m, f, *spots[nm]) for nm in names])
    Xn[names.index("nan"), 1] = np.nan
    m.X = np.concatenate([m.X, Xn.reshape(-1)])
    m.point_flags = np.concatenate([m.point_flags, np.zeros(len(names), dtype=np.int32)])
    m.point_uncertainty = np.concatenate([m.point_uncertainty, np.ones(len(names))])
    m.X_true = None
    desc = {nm: _random_desc(rng, 1)[0] for nm in names}
    desc["tie_lo"] = desc["tie_hi"].copy()                       # the same descriptor twice in one window
    desc["alike_b"] = desc["alike_a"] ^ np.array([0xF, 0, 0, 0], dtype=np.uint64)      # 4 bits apart
    cam = m.frame_camera[f]
    uv, ok, _ = project(m.q[4 * f:4 * f + 4], m.t[3 * f:3 * f + 3], m.k[7 * cam:7 * cam + 7], Xn)
    px = {nm: uv[i] for i, nm in enumerate(names)}
    assert not ok[names.index("behind")] and px["left"][0] < -NEAR and 0 < px["left"][1] < HEIGHT
    assert np.hypot(*(px["tie_hi"] - px["tie_lo"])) < 6 and np.hypot(*(px["seen"] - px["unseen"])) < 8
    assert np.hypot(*(px["alike_a"] - px["alike_b"])) < 8
    # the frame observes "seen" (its observation is appended; cases toggle obs_disabled of it)
    m.obs_pt = np.concatenate([m.obs_pt, px["seen"]])
    m.obs_frame = np.concatenate([m.obs_frame, np.array([f], dtype=np.int32)])
    m.obs_point = np.concatenate([m.obs_point, np.array([idx["seen"]], dtype=np.int32)])
    m.obs_disabled = np.concatenate([m.obs_disabled, np.zeros(1, dtype=np.int32)])
    m.obs_error = np.concatenate([m.obs_error, np.zeros(2)])

    def bits(lo, n):      # n set bits starting at bit lo of word 1 (clear of the 4 bits alike_a and alike_b differ in)
        return np.array([0, ((1 << n) - 1) << lo, 0, 0], dtype=np.uint64)

    kps = [  # (name, pixel, descriptor)
        ("at_behind", px["behind"], desc["behind"]),
        ("at_left", px["left"] + [3.0, 4.0], desc["left"] ^ bits(0, 2)),
        ("empty", np.array([600.0, 30.0]), _random_desc(rng, 1)[0]),
        ("single", px["single"] + [-3.0, 4.0], desc["single"] ^ bits(0, 7)),
        ("nan_x", np.array([np.nan, 100.0]), desc["single"]),
        ("inf_y", px["single"] * [1.0, np.inf], desc["single"]),
        ("tie", 0.5 * (px["tie_hi"] + px["tie_lo"]) + [0.0, 1.0], desc["tie_hi"].copy()),
        ("tie_flipped", 0.5 * (px["tie_hi"] + px["tie_lo"]) + [0.0, -1.5], desc["tie_hi"] ^ bits(0, 3)),
        ("near_seen", px["seen"] + [1.0, 1.0], desc["seen"] ^ bits(0, 2)),
        ("claim_far", px["shared"] + [2.0, 0.0], desc["shared"] ^ bits(0, 5)),
        ("claim_near", px["shared"] + [-2.0, 0.5], desc["shared"] ^ bits(8, 3)),
        ("claim_eq_first", px["shared_eq"] + [0.0, 2.0], desc["shared_eq"] ^ bits(0, 4)),
        ("claim_eq_second", px["shared_eq"] + [0.0, -2.0], desc["shared_eq"] ^ bits(8, 4)),
        ("alike", px["alike_a"] + [0.5, 0.5], desc["alike_a"] ^ bits(0, 20)),
        ("far", px["far"] + [5.0, 0.0], desc["far"] ^ bits(0, 60)),                     # 60 <= max_dist: accepted
        ("too_far", px["far"] + [-5.0, 1.0], desc["far"] ^ bits(0, 62) ^ np.array([0xFF, 0, 0, 0], dtype=np.uint64)),
    ]
    # "unseen" is 40 bits from the keypoint near "seen": the best candidate once "seen" is excluded
    desc["unseen"] = kps[8][2] ^ bits(20, 40)
    order = ["far", "tie_lo", "alike_b", "unseen", "left", "nan", "behind", "seen", "single", "shared_eq", "alike_a",
             "tie_hi", "shared"]       # tie_lo has the lower position and the higher map index
    points = np.array([idx[nm] for nm in order], dtype=np.int32)
    point_desc = np.stack([desc[nm] for nm in order])
    xy = np.stack([np.asarray(k[1], dtype=np.float64) for k in kps])
    kd = np.stack([k[2] for k in kps])
    return m, idx, points, point_desc, [k[0] for k in kps], xy, kd


def planted(kind="skip_on"):
    """One planted case.  kind: "skip_on" (the defaults), "skip_off", "obs_disabled" (skip_observed on, the planted
    observation disabled), "bounded" (skip_on with the image bounds).  Listed: the planted frame, a frame without
    keypoints, and frame 7 with a few keypoints that see none of the planted points nearby."""
    m, idx, points, point_desc, names, xy, kd = _planted_base()
    m = m.copy()
    if kind == "obs_disabled":
        m.obs_disabled[-1] = 1
    opt = options(skip_observed=0 if kind == "skip_off" else 1)
    if kind == "bounded":
        opt.update(width=WIDTH, height=HEIGHT)
    rng = np.random.default_rng(3)
    other = (np.stack([rng.uniform(0, WIDTH, 5), rng.uniform(0, HEIGHT, 5)], 1), _random_desc(rng, 5))
    none = (np.zeros((0, 2)), np.zeros((0, 4), dtype=np.uint64))
    c = SimpleNamespace(m=m, frames=[PLANT_FRAME, 2, 7], keypoints=[(xy, kd), none, other], points=points,
                        point_desc=point_desc, options=opt)
    c.kp_names, c.idx = names, idx
    return c


CASE_NAMES = ("c1", "c1_skip_off", "c1_bounded", "long", "planted_skip_on", "planted_skip_off", "planted_obs_disabled",
              "planted_bounded")


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "c1":
        return generated(False, (3, 8))
    if name == "c1_skip_off":
        return generated(False, (3, 8), skip_observed=0)
    if name == "c1_bounded":
        return generated(False, (8, 3, 5), skip_observed=0, width=WIDTH, height=HEIGHT)
    if name == "long":
        return generated(True, (3, 8), skip_observed=0)
    assert name.startswith("planted_")
    return planted(name[len("planted_"):])


@functools.lru_cache(maxsize=None)
def expected(name):
    """The reference answer of a named case, computed once and shared (treat it as read-only)."""
    return reference(case(name))
