"""Inputs of the tracker's window / odd-size / deep-pyramid tests, and the oracle's answers on them.  Test material
only: nothing here is a path of the library, and this file holds no tests.

The device tracker (csrc/tracker.hip) instantiates k_track_fb, k_track_one and k_find_matches per
NK = ceil(W^2 / 64), W = 1..16, and stages a 40 x 40 tile of the destination level in LDS on levels of at least 40 x 40.
The cases put a tracking run on every NK, on even windows (0.5 W and (W - 1) / 2 fall on different halves of a pixel),
on W = 8 (64 pixels: no idle lane) and W = 16 (256 pixels: every slot live), and on pyramids whose levels are odd,
exactly 40 or 41 wide, smaller than the window, or 7 and 8 deep.

A case is built from
  frames   slamgpu.video.make_frames(2, w, h): frame 1 is frame 0 moved by a known translation and rotation;
  points   seed_points(n, w, h, border) plus five edge points: two on the left / right border (out of bounds at entry
           when the start falls outside), two in the corners (zero-filled and border-replicated patches), one inside
           the zero-fill band of the window (W / 2 - 0.25, W / 2 + 0.25);
  starts   points + N(0, 0.5) in float32;
  levels   drawn per feature from the case's level set (the largest is retry_levels, so those features have no retry).
Every draw comes from one generator per case with a fixed seed.

Cases A ("a_wW"): 640 x 480, depth 6, 240 seeds (border 10), levels {3, 6}, retry 6, W in A_WINDOWS.
Cases B ("b_WxH_wW"): 120 seeds (border 6), W in B_WINDOWS, on
  321 x 241, depth 8, levels {3, 8}, retry 8: 321x241, 161x121, 81x61 (staged, the tile clamped on every side), 41x31
             (41 wide, unstaged), 21x16, 11x8, 6x4, 3x2: every level odd in one size at least;
  160 x 163, depth 4, levels {2, 4}, retry 4: 160x163, 80x82, 40x41 (the tile is the whole width), 20x21;
  211 x 97,  depth 6, levels {1, 3, 6}, retry 6: ..., 14x7, 7x4: levels smaller than the window.

tests/test_tracker_cases.py holds the cases to conditions on the oracle alone, so that a device comparison on them
cannot pass by being trivial; tests/test_tracker_windows_gpu.py compares the device with expected()."""
import functools
import os
from types import SimpleNamespace

import numpy as np

import oracle
import oracle_matcher as om
from slamgpu.video import SEQ_K, make_frames, seed_points, sequence_mark, sequence_pose, sequence_true_t

A_WINDOWS = (2, 8, 9, 10, 11, 12, 14, 15, 16)
B_WINDOWS = (9, 13, 16)
B_IMAGES = {   # (w, h): depth, level set, retry_levels
    (321, 241): (8, (3, 8), 8),
    (160, 163): (4, (2, 4), 4),
    (211, 97): (6, (1, 3, 6), 6),
}
# The generator seed of each case's starts and levels: the lowest one found at which the case meets every condition of
# tests/test_tracker_cases.py.  The scarce condition is five features that are rejected although they were retried:
# the seeded features nearly all track and two of the edge points are accepted at most windows, so at some windows it
# takes the three other edge points drawn with a low level and two unlucky features besides (at W = 15 any one of
# them fails its retry at about one seed in 230, hence a_w15's seed).
SEEDS = {
    "a_w2": 1, "a_w8": 1, "a_w9": 24856, "a_w10": 1, "a_w11": 43, "a_w12": 15, "a_w14": 15, "a_w15": 3960165, "a_w16": 1,
    "b_321x241_w9": 1, "b_321x241_w13": 58, "b_321x241_w16": 1,
    "b_160x163_w9": 4645, "b_160x163_w13": 1, "b_160x163_w16": 1,
    "b_211x97_w9": 68, "b_211x97_w13": 661, "b_211x97_w16": 1,
}
A_NAMES = tuple("a_w%d" % W for W in A_WINDOWS)
B_NAMES = tuple("b_%dx%d_w%d" % (w, h, W) for (w, h) in B_IMAGES for W in B_WINDOWS)
CASE_NAMES = A_NAMES + B_NAMES
NTHREADS = min(16, os.cpu_count() or 1)


def nk(W):
    """Patch pixels per lane of a W x W window: the kernels' template argument."""
    return (W * W + 63) // 64


@functools.lru_cache(maxsize=None)
def frames(w, h):
    return tuple(make_frames(2, w, h))


def edge_points(w, h, W):
    return np.array([[0.005, h / 2], [w - 0.001, h / 3], [3, 3], [w - 3.5, h - 2.5], [W / 2 - 0.25, W / 2 + 0.25]],
                    np.float32)


def _build(name, w, h, W, depth, level_set, retry, nseed, border, seed):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([seed_points(nseed, w, h, border), edge_points(w, h, W)]).astype(np.float32)
    start = (pts + rng.normal(0, 0.5, pts.shape)).astype(np.float32)
    k = len(level_set)   # the deepest level (= retry_levels) with probability 0.3, as test_tracker_gpu.py draws 6 against 3
    levels = rng.choice(np.array(level_set, np.int32), len(pts), p=[0.7 / (k - 1)] * (k - 1) + [0.3]).astype(np.int32)
    return SimpleNamespace(name=name, w=w, h=h, frames=frames(w, h), pts=pts, start=start, levels=levels, window=W,
                           depth=depth, retry_levels=retry, level_set=level_set)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case: frames (2 images), pts, start, levels, window, depth, retry_levels."""
    if name in A_NAMES:
        W = int(name[3:])
        return _build(name, 640, 480, W, 6, (3, 6), 6, 240, 10, SEEDS[name])
    if name not in B_NAMES:
        raise KeyError(name)
    size, win = name[2:].split("_w")
    w, h = (int(v) for v in size.split("x"))
    depth, level_set, retry = B_IMAGES[(w, h)]
    return _build(name, w, h, int(win), depth, level_set, retry, 120, 6, SEEDS[name])


@functools.lru_cache(maxsize=None)
def pyramids(w, h, depth):
    """The oracle's pyramids of the two frames: (flat levels of frame 0, of frame 1, dims)."""
    f0, f1 = frames(w, h)
    p0, dims = oracle.make_pyramid(f0, depth)
    p1, _ = oracle.make_pyramid(f1, depth)
    for a in (p0, p1, dims):
        a.setflags(write=False)
    return p0, p1, dims


@functools.lru_cache(maxsize=None)
def _expected(name, order):
    c = case(name)
    p0, p1, dims = pyramids(c.w, c.h, c.depth)
    oracle.set_sum_order(order)
    try:
        out, acc, its = oracle.track_fb(p0, p1, dims, c.window, c.pts, c.start, c.levels, nthreads=NTHREADS,
                                        retry_levels=c.retry_levels)
    finally:
        oracle.set_sum_order(0)
    for a in (out, acc, its):
        a.setflags(write=False)
    return out, acc, its


def expected(name):
    """oracle.track_fb on the case: (to_xy, accepted, iterations).  Computed once, read-only."""
    return _expected(name, 0)


def expected_sequential_sums(name):
    """The same with the oracle's patch sums in the reference's left-to-right order instead of the lane tree."""
    return _expected(name, 1)


# ------------------------------------------------------------------------------------------------ Matcher::Track
def run_oracle(frames_, window=om.WINDOW):
    """The sequential restatement of Matcher::Track over a slamgpu.video.matcher_sequence() prefix: (map, matcher,
    per-frame stats)."""
    omap = om.OracleMap(SEQ_K, [], [], [])
    mt = om.OracleMatcher(window=window)
    log = []
    for i, img in enumerate(frames_):
        q, t = sequence_pose(i)
        omap.q.append(list(q))
        omap.t.append(list(t))
        omap.frame_camera.append(0)
        omap.obs[i] = []
        omap.keyframe.append(0)
        sequence_mark(i, omap.flags, omap.uncertainty, len(omap.X))

        def upd(i=i):   # Matcher::Track's update_frames: correct the new frame's pose, report it updated
            omap.t[i] = list(sequence_true_t(i))
            return i % 2 == 1
        assert mt.Track(img, i, omap, upd)
        log.append(dict(mt.last_stats))
    return omap, mt, log
