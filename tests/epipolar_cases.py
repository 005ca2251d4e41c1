"""Scenes and the numpy reference of sg_slam_match_epipolar (include/slamgpu.h).  Test material only: nothing here is a
path of the library.

c1_*: match_cases.scene(False), that is make_config("C1", noise=0, outlier_frac=0, perturb=False) with camera 1's
intrinsics overwritten by match_cases.K_DISTORTED and its pixels recomputed.  Pairs (0,1), (0,2), (1,3), (0,9); a frame's
keypoints are all its observation pixels (shared with the other frame or not) with the landmark's descriptor after
Binomial(256, 0.03) bit flips, plus 300 distractors with fresh descriptors at random pixels, random levels 0..3, all
shuffled.  Run with and without levels, with and without min_parallax.

shapes: one pose pair listed once per (na, nb) of NA x NB, uniform random pixels, a 25 px gate, and descriptors of 12
random bits so that distances tie often (ties are decided by the b index, across waves, tiles and slices).

planted: hand-placed keypoints in pair (0, 1), one item per rule of the contract (planted()), a zero-baseline pair, the
same pair listed again with other keypoints, and a pair without a keypoints.

The reference (reference()) is the contract written plainly.  Its `off` argument switches single rules off, for the
tests that show each planted item bites."""
import functools
from types import SimpleNamespace

import numpy as np

import match_cases as mc
from slamgpu.scene import HEIGHT, WIDTH, quat_to_matrix

CHUNK = 64           # kEpiChunk of csrc/epipolar_plan.h (held equal by test_epipolar_plan.py, as the next two)
TILE = 256           # kEpiTile
SLICE = 512          # kEpiSlice
NEAR = 1e-9          # relative: no decision of a case comes this close to its threshold
C1_PAIRS = ((0, 1), (0, 2), (1, 3), (0, 9))
MIN_PARALLAX = 0.02  # rad, where a case uses the parallax test
NA = (1, 63, 64, 65, 130)
NB = (1, 3, 255, 256, 257, SLICE, SLICE + 1, 2 * SLICE + 76)
ARRAYS = ("match", "best_kp", "best_dist", "second_dist", "num_candidates")
COUNTS = ("num_a", "num_b", "num_with_candidates", "num_matched", "degenerate")


# ------------------------------------------------------------------------------------------------ the reference
def undistort(k, px):
    """UndistortPixel of csrc/project_math.h on rows of pixels."""
    px = np.asarray(px, dtype=np.float64).reshape(-1, 2)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        xd, yd = (px[:, 0] - k[5]) / k[3], (px[:, 1] - k[6]) / k[4]
        rd = np.sqrt(xd * xd + yd * yd)
        r = rd.copy()
        for _ in range(8):
            r2 = r * r
            f = r * (1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) - rd
            df = 1.0 + r2 * (3.0 * k[0] + r2 * (5.0 * k[1] + r2 * (7.0 * k[2])))
            r = r - f / df
        s = r / rd
        out = np.stack([xd * s, yd * s], 1)
    out[rd == 0] = 0.0
    return out


def distort(k, x):
    """Project's image half: plane coordinates -> pixels."""
    x = np.asarray(x, dtype=np.float64)
    r2 = x[0] * x[0] + x[1] * x[1]
    d = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))
    return np.array([x[0] * d * k[3] + k[5], x[1] * d * k[4] + k[6]])


def pair_record(m, fa, fb):
    """Step 1 of the contract: R, tr, E, ifa, ifb, the two cameras and the degenerate flag."""
    with np.errstate(invalid="ignore", over="ignore"):
        Ra, Rb = quat_to_matrix(m.q[4 * fa:4 * fa + 4]), quat_to_matrix(m.q[4 * fb:4 * fb + 4])
        R = Rb @ Ra.T
        tr = Rb @ (m.t[3 * fa:3 * fa + 3] - m.t[3 * fb:3 * fb + 3])
        tx = np.array([[0.0, -tr[2], tr[1]], [tr[2], 0.0, -tr[0]], [-tr[1], tr[0], 0.0]])
        E = tx @ R
    ka, kb = m.k[7 * m.frame_camera[fa]:][:7], m.k[7 * m.frame_camera[fb]:][:7]
    finite = np.isfinite(E).all() and np.isfinite(R).all() and np.isfinite(tr).all()
    return SimpleNamespace(R=R, tr=tr, E=E, ifa=1.0 / ka[3:5], ifb=1.0 / kb[3:5], ka=ka, kb=kb,
                           degenerate=int(not finite or not E.any()))


def pair_tests(rec, axy, alv, bxy, blv, opt, off=()):
    """Steps 2 and 3 on one pair: the candidate matrix (na, nb) and, for the bounds test, the smallest relative
    distance of any decision that was reached from its threshold: gate, det, the depth numerators, parallax."""
    xa, xb = undistort(rec.ka, axy), undistort(rec.kb, bxy)
    fa = np.concatenate([xa, np.ones((len(xa), 1))], 1)
    fb = np.concatenate([xb, np.ones((len(xb), 1))], 1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        ln, g = fa @ rec.E.T, fa @ rec.R.T
        na = (ln[:, 0] * rec.ifb[0]) ** 2 + (ln[:, 1] * rec.ifb[1]) ** 2
        mm = fb @ rec.E
        nb = (mm[:, 0] * rec.ifa[0]) ** 2 + (mm[:, 1] * rec.ifa[1]) ** 2
        r = xb[None, :, 0] * ln[:, None, 0] + xb[None, :, 1] * ln[:, None, 1] + ln[:, None, 2]
        den = na[:, None] + nb[None, :]
        L = np.zeros((len(xa), len(xb)))
        if alv is not None and "level" not in off:
            L = np.maximum(np.asarray(alv)[:, None], np.asarray(blv)[None, :]).astype(np.float64)
        thr = (opt["tol_px"] * opt["tol_px"]) * 4.0 ** L * den
        gate = (den > 0) & (r * r <= thr)
        gaps = dict(gate=_least(np.abs(r * r - thr) / thr, np.isfinite(r) & (den > 0)))
        gf = g @ fb.T
        gg, ff = (g * g).sum(1)[:, None], (fb * fb).sum(1)[None, :]
        gt, ft = (g @ rec.tr)[:, None], (fb @ rec.tr)[None, :]
        det = gg * ff - gf * gf
        da, db = -gt * ff + gf * ft, gg * ft - gf * gt
        depth = (det > 0) & (da > 0) & (db > 0)
        gaps["det"] = _least(np.abs(det) / (gg * ff), gate)
        gaps["depth"] = min(_least(np.abs(da) / (np.abs(gt * ff) + np.abs(gf * ft)), gate & (det > 0)),
                            _least(np.abs(db) / (np.abs(gg * ft) + np.abs(gf * gt)), gate & (det > 0)))
        cand = gate if "depth" in off else gate & depth
        gaps["parallax"] = np.inf
        if opt["min_parallax"] > 0:
            c = np.cross(g[:, None, :], fb[None, :, :])
            par = np.arctan2(np.sqrt((c * c).sum(2)), gf)
            gaps["parallax"] = _least(np.abs(par - opt["min_parallax"]) / opt["min_parallax"], gate & depth)
            if "parallax" not in off:
                cand = cand & (par >= opt["min_parallax"])
    return cand, gaps


def _least(v, where):
    v = v[where & np.isfinite(v)]
    return float(v.min()) if v.size else np.inf


def resolve(bk, bd, sd, opt, off=()):
    """Step 5: acceptance and the one-to-one rule within one pair."""
    accept = (bk >= 0) & (bd <= opt["max_dist"])
    if "ratio" not in off:
        accept &= (sd < 0) | (100 * bd.astype(np.int64) <= opt["ratio_percent"] * sd.astype(np.int64))
    match = np.where(accept, bk, -1).astype(np.int32)
    if "unique" not in off:
        for j in np.unique(match[match >= 0]):
            who = np.flatnonzero(match == j)
            keep = who[np.lexsort((who, bd[who]))[0]]
            match[who[who != keep]] = -1
    return match


def reference(case, off=()):
    """The contract on one case, per listed pair: a dict of the five int32 arrays, the five counts of
    sg_epipolar_result, the candidate matrix `cand` and the margins `gaps`.  off: rules switched off, any of "tie",
    "ratio", "unique", "depth", "parallax", "level"."""
    out = []
    for (fa, fb), ka, kb in zip(case.pairs, case.keypoints_a, case.keypoints_b):
        axy, ad = np.asarray(ka[0], dtype=np.float64).reshape(-1, 2), np.asarray(ka[1], dtype=np.uint64).reshape(-1, 4)
        bxy, bdsc = np.asarray(kb[0], dtype=np.float64).reshape(-1, 2), np.asarray(kb[1], dtype=np.uint64).reshape(-1, 4)
        alv, blv = (ka[2], kb[2]) if case.levels else (None, None)
        rec = pair_record(case.m, fa, fb)
        K = len(axy)
        bk, bd, sd = (np.full(K, -1, dtype=np.int32) for _ in range(3))
        nc = np.zeros(K, dtype=np.int32)
        cand, gaps = np.zeros((K, len(bxy)), dtype=bool), dict(gate=np.inf, det=np.inf, depth=np.inf, parallax=np.inf)
        if not rec.degenerate and K and len(bxy):
            cand, gaps = pair_tests(rec, axy, alv, bxy, blv, case.options, off)
        for i in range(K):
            w = np.flatnonzero(cand[i])
            nc[i] = len(w)
            if len(w) == 0:
                continue
            h = mc.popcount(bdsc[w] ^ ad[i][None, :])
            order = np.lexsort((-w if "tie" in off else w, h))
            bk[i], bd[i] = w[order[0]], h[order[0]]
            if len(w) > 1:
                sd[i] = h[order[1]]
        match = resolve(bk, bd, sd, case.options, off)
        out.append(dict(match=match, best_kp=bk, best_dist=bd, second_dist=sd, num_candidates=nc, num_a=K,
                        num_b=len(bxy), num_with_candidates=int((nc > 0).sum()), num_matched=int((match >= 0).sum()),
                        degenerate=rec.degenerate, cand=cand, gaps=gaps))
    return out


def options(**kw):
    o = dict(tol_px=2.0, min_parallax=0.0, max_dist=64, ratio_percent=80)
    o.update(kw)
    return o


def _case(m, pairs, kps_a, kps_b, levels, truth=None, **opt):
    return SimpleNamespace(m=m, pairs=[tuple(p) for p in pairs], keypoints_a=kps_a, keypoints_b=kps_b, levels=levels,
                           truth=truth, options=options(**opt))


def call_keypoints(case, side):
    """The case's keypoints of one side ("a" or "b") as Slam.MatchEpipolar takes them: with levels or without."""
    kps = case.keypoints_a if side == "a" else case.keypoints_b
    return [k if case.levels else k[:2] for k in kps]


# ------------------------------------------------------------------------------------------------ generated scenes
def frame_keypoints(m, desc, f, seed, distract=300):
    """All observation pixels of frame f with flipped descriptors, and distractors, shuffled: pixels, descriptors,
    levels and the map point behind each keypoint (-1 for a distractor)."""
    rng = np.random.default_rng(seed)
    sel = np.flatnonzero(m.obs_frame == f)
    xy = np.concatenate([m.obs_pt.reshape(-1, 2)[sel],
                         np.stack([rng.uniform(0, WIDTH, distract), rng.uniform(0, HEIGHT, distract)], 1)])
    kd = np.concatenate([mc._flip(rng, desc[m.obs_point[sel]]), mc._random_desc(rng, distract)])
    pid = np.concatenate([m.obs_point[sel].astype(np.int64), np.full(distract, -1)])
    lv = rng.integers(0, 4, len(xy)).astype(np.int32)
    order = rng.permutation(len(xy))
    return xy[order], kd[order], lv[order], pid[order]


def c1(levels, min_parallax):
    m, desc = mc.scene(False)
    kps_a, kps_b, truth = [], [], []
    for i, (fa, fb) in enumerate(C1_PAIRS):
        a = frame_keypoints(m, desc, fa, 3000 + 2 * i)
        b = frame_keypoints(m, desc, fb, 3001 + 2 * i)
        ia, jb = np.nonzero((a[3][:, None] == b[3][None, :]) & (a[3][:, None] >= 0))
        kps_a.append(a[:3])
        kps_b.append(b[:3])
        truth.append(SimpleNamespace(ia=ia, jb=jb, point=a[3][ia]))
    return _case(m, C1_PAIRS, kps_a, kps_b, levels, truth, min_parallax=min_parallax)


def shapes():
    m, _ = mc.scene(False)
    rng = np.random.default_rng(11)

    def side(n):
        d = np.zeros((n, 4), dtype=np.uint64)
        d[:, 0] = rng.integers(0, 2 ** 12, n)
        return np.stack([rng.uniform(0, WIDTH, n), rng.uniform(0, HEIGHT, n)], 1), d, np.zeros(n, dtype=np.int32)

    combos = [(na, nb) for na in NA for nb in NB]
    return _case(m, [(2, 3)] * len(combos), [side(na) for na, _ in combos], [side(nb) for _, nb in combos], False,
                 tol_px=25.0, max_dist=256, ratio_percent=100)


# ------------------------------------------------------------------------------------------------ the planted scene
PLANT_PAIR = (0, 1)          # frame 0 has camera 1, the distorted one
ZERO_PAIR = (4, 5)           # given one centre below


def _bits(lo, n):            # n set bits starting at bit lo of word 1
    return np.array([0, ((1 << n) - 1) << lo, 0, 0], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def _planted_base():
    m0, _ = mc.scene(False)
    m = m0.copy()
    m.t[3 * ZERO_PAIR[1]:3 * ZERO_PAIR[1] + 3] = m.t[3 * ZERO_PAIR[0]:3 * ZERO_PAIR[0] + 3]   # a zero baseline
    assert m.frame_camera[PLANT_PAIR[0]] == 1
    rec = pair_record(m, *PLANT_PAIR)
    rng = np.random.default_rng(41)
    px_b = 1.0 / abs(rec.kb[4])          # one pixel of frame b in plane coordinates, across the (horizontal) lines

    def a_pixel(x, y):
        return distort(rec.ka, (x, y))

    def b_pixel(x, y, depth, along=0.0, across=0.0):
        """Where frame b sees the point at `depth` along a's bearing (x, y, 1), moved by pixels along and across the
        epipolar line (the pair is a stereo pair: its lines are the rows of b)."""
        p = rec.R @ (depth * np.array([x, y, 1.0])) + rec.tr
        return distort(rec.kb, (p[0] / p[2] + along * px_b, p[1] / p[2] + across * px_b))

    D = [mc._random_desc(rng, 1)[0] for _ in range(10)]
    A = [  # (name, pixel, descriptor, level)
        ("tie", a_pixel(0.10, -0.40), D[0].copy(), 0),
        ("alike", a_pixel(0.20, -0.30), D[1] ^ _bits(0, 20), 0),
        ("claim_far", a_pixel(0.00, -0.20), D[2] ^ _bits(0, 5), 0),
        ("claim_near", a_pixel(0.00, -0.20) + [0.5, 0.0], D[2] ^ _bits(8, 3), 0),
        ("behind", a_pixel(0.15, -0.10), D[3] ^ _bits(0, 2), 0),
        ("flat", a_pixel(0.25, 0.00), D[4] ^ _bits(0, 2), 0),
        ("level_b", a_pixel(0.05, 0.10), D[5] ^ _bits(0, 2), 0),
        ("level_a", a_pixel(0.05, -0.50), D[6] ^ _bits(0, 2), 2),
        ("nan_x", np.array([np.nan, 100.0]), D[0].copy(), 0),
        ("inf_y", np.array([100.0, np.inf]), D[0].copy(), 0),
        ("single", a_pixel(0.30, 0.20), D[7] ^ _bits(0, 7), 0),
        ("too_far", a_pixel(0.10, 0.30), D[8] ^ _bits(0, 62) ^ np.array([0xFF, 0, 0, 0], dtype=np.uint64), 0),
        ("empty", a_pixel(0.20, 0.40), D[9].copy(), 0),
    ]
    B = [  # tie_lo has the lower index
        ("single", b_pixel(0.30, 0.20, 2000.0, across=1.0), D[7].copy(), 0),
        ("tie_lo", b_pixel(0.10, -0.40, 2500.0, along=0.3), D[0].copy(), 0),
        ("alike_b", b_pixel(0.20, -0.30, 1800.0, along=-1.0), D[1] ^ np.array([0xF, 0, 0, 0], dtype=np.uint64), 0),
        ("nan_y", np.array([200.0, np.nan]), D[0].copy(), 0),
        ("behind", b_pixel(0.15, -0.10, -2000.0), D[3].copy(), 0),
        ("shared", b_pixel(0.00, -0.20, 3000.0), D[2].copy(), 0),
        ("flat", b_pixel(0.25, 0.00, 1e6), D[4].copy(), 0),
        ("level_b", b_pixel(0.05, 0.10, 2200.0, across=4.5), D[5].copy(), 1),
        ("level_a", b_pixel(0.05, -0.50, 2200.0, across=-9.0), D[6].copy(), 0),
        ("alike_a", b_pixel(0.20, -0.30, 1800.0), D[1].copy(), 0),
        ("tie_hi", b_pixel(0.10, -0.40, 2500.0, along=-0.3), D[0].copy(), 0),
        ("too_far", b_pixel(0.10, 0.30, 2600.0), D[8].copy(), 0),
    ]
    pack = lambda rows: (np.stack([np.asarray(r[1], dtype=np.float64) for r in rows]),   # noqa: E731
                         np.stack([r[2] for r in rows]), np.array([r[3] for r in rows], dtype=np.int32))
    return m, [r[0] for r in A], pack(A), [r[0] for r in B], pack(B)


def planted(full=True):
    """full: levels given and min_parallax = MIN_PARALLAX; otherwise neither.  Pairs: the planted pair; the
    zero-baseline pair with the same keypoints; the planted pair again with the first five a keypoints and the b
    keypoints reversed; a pair without a keypoints."""
    m, a_names, a, b_names, b = _planted_base()
    head = tuple(x[:5] for x in a)
    rev = tuple(x[::-1] for x in b)
    none = (np.zeros((0, 2)), np.zeros((0, 4), dtype=np.uint64), np.zeros(0, dtype=np.int32))
    c = _case(m, [PLANT_PAIR, ZERO_PAIR, PLANT_PAIR, (3, 2)], [a, a, head, none], [b, b, rev, tuple(x[:3] for x in b)],
              full, min_parallax=MIN_PARALLAX if full else 0.0)
    c.a_names, c.b_names = a_names, b_names
    return c


CASE_NAMES = ("c1", "c1_levels", "c1_parallax", "c1_levels_parallax", "shapes", "planted", "planted_plain")


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("c1"):
        return c1("levels" in name, MIN_PARALLAX if "parallax" in name else 0.0)
    if name == "shapes":
        return shapes()
    return planted(name == "planted")


@functools.lru_cache(maxsize=None)
def expected(name):
    """The reference answer of a named case, computed once and shared (treat it as read-only)."""
    return reference(case(name))
