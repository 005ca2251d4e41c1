"""The numpy reference of sg_tracker_describe (include/slamgpu.h) and the cases of its tests.  Test material only:
nothing here is a path of the library.

reference_level() is the contract written plainly on one level array: the centre pixel and the border rule in fp32, the
two first moments of the radius-15 disc in fp64, the bin as the nearest multiple of 2 pi / 32 to atan2(m01, m10), the
256 comparisons of the pattern table, which it imports from tools/make_brief_pattern.py.  Beside desc, angle_bin and
status it returns a gap per keypoint: (the angular distance of atan2(m01, m10) to the nearest bin boundary) x
hypot(m10, m01) / sum (|u| + |v|) I.  Re-ordering an fp64 sum of 709 exact products moves that quantity by about
709 x 2^-53 = 8e-14, so a keypoint with a gap of GAP = 1e-9 or more has one right answer, whatever the order of the
sums; the bin is the only decision of the contract that rounding can touch.  tests/test_describe_reference_bounds.py
holds every case below to that gap.

Cases: device_case(name) gives an image, a depth and 257 keypoints for tests/test_describe_gpu.py (its smaller calls
take prefixes of them); texture_case() is 600 seed points of the 640 x 480 texture on its oracle pyramid."""
import functools
import importlib.util
import os
from types import SimpleNamespace

import numpy as np

from slamgpu.video import make_frames, seed_points


def load_pattern_tool():
    """tools/make_brief_pattern.py as a module, loaded from its file (tools/ is not a package)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "make_brief_pattern.py")
    spec = importlib.util.spec_from_file_location("make_brief_pattern", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pattern = load_pattern_tool().pattern

GAP = 1e-9
R = 15
BINS = 32
_V, _U = np.mgrid[-R:R + 1, -R:R + 1]
_IN = _U * _U + _V * _V <= R * R
DU, DV = _U[_IN].astype(np.int64), _V[_IN].astype(np.int64)      # the 709 disc offsets
assert len(DU) == 709


# ------------------------------------------------------------------------------------------------ the reference
def centres(xy, level, w, h):
    """(cx, cy, ok) of level-0 points xy (n, 2) on pyramid level `level` of size w x h: fp32 as the contract."""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(xy * np.float32(2.0 ** -level) + np.float32(0.5))
        ok = np.isfinite(xy).all(1) & (f[:, 0] >= R) & (f[:, 0] <= w - 1 - R) & (f[:, 1] >= R) & (f[:, 1] <= h - 1 - R)
    c = np.where(ok[:, None], f, 0).astype(np.int64)
    return c[:, 0], c[:, 1], ok


def reference_level(img, xy, level=0, steer=True):
    """The contract on level array img (h, w) float32 for level-0 points xy: dict of desc uint64 (n, 4), angle_bin,
    status (int32), gap (float64; inf where no rounding can matter: refused keypoints, zero moments) and the moments.
    steer=False forces bin 0 for the bits (the unsteered descriptor of the steering test)."""
    img = np.asarray(img, dtype=np.float32)
    h, w = img.shape
    cx, cy, ok = centres(xy, level, w, h)
    n = len(cx)
    desc = np.zeros((n, 4), dtype=np.uint64)
    ang = np.full(n, -1, dtype=np.int32)
    gap = np.full(n, np.inf)
    m10, m01 = np.zeros(n), np.zeros(n)
    k = np.flatnonzero(ok)
    if len(k):
        I = img[cy[k, None] + DV[None, :], cx[k, None] + DU[None, :]].astype(np.float64)
        a, b = (I * DU).sum(1), (I * DV).sum(1)
        m10[k], m01[k] = a, b
        step = 2.0 * np.pi / BINS
        t = np.arctan2(b, a) / step
        q = np.rint(t)
        bins = np.where((a == 0) & (b == 0), 0, q.astype(np.int64) % BINS)
        norm = (I * (np.abs(DU) + np.abs(DV))).sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            g = (0.5 - np.abs(t - q)) * step * np.hypot(a, b) / norm
        gap[k] = np.where((a == 0) & (b == 0), np.inf, g)
        ang[k] = bins
        T = pattern()[bins if steer else np.zeros_like(bins)].astype(np.int64)      # (m, 256, 4)
        pa = img[cy[k, None] + T[:, :, 1], cx[k, None] + T[:, :, 0]]
        pb = img[cy[k, None] + T[:, :, 3], cx[k, None] + T[:, :, 2]]
        desc[k] = np.packbits(pa < pb, axis=1, bitorder="little").view("<u8").reshape(-1, 4)
    return dict(desc=desc, angle_bin=ang, status=np.where(ok, 0, 1).astype(np.int32), gap=gap, m10=m10, m01=m01)


def reference(levels_img, xy, levels=None, steer=True):
    """reference_level over keypoints on several levels of one pyramid (levels_img: list of level arrays)."""
    xy = np.asarray(xy, dtype=np.float32).reshape(-1, 2)
    n = len(xy)
    lv = np.zeros(n, dtype=np.int64) if levels is None else np.asarray(levels, dtype=np.int64)
    out = dict(desc=np.zeros((n, 4), dtype=np.uint64), angle_bin=np.full(n, -1, dtype=np.int32),
               status=np.ones(n, dtype=np.int32), gap=np.full(n, np.inf), m10=np.zeros(n), m01=np.zeros(n))
    for l in np.unique(lv):
        sel = np.flatnonzero(lv == l)
        r = reference_level(levels_img[l], xy[sel], int(l), steer)
        for key in out:
            out[key][sel] = r[key]
    return out


def popcount(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape[:-1] + (32,)), axis=-1).sum(-1).astype(np.int64)


def hamming(a, b):
    """All-pairs Hamming distances of descriptor rows a (n, 4) and b (m, 4)."""
    return popcount(a[:, None, :] ^ b[None, :, :])


# ------------------------------------------------------------------------------------------------ cases
def pyramid_dims(w, h, depth):
    out = []
    for _ in range(depth):
        out.append((w, h))
        w, h = (w + 1) // 2, (h + 1) // 2
    return out


def oracle_levels(img, depth):
    import oracle
    flat, dims = oracle.make_pyramid(img, depth)
    return oracle.pyramid_levels(flat, dims)


DEVICE_CASES = {"odd": (161, 121, 3),       # levels 161 x 121, 81 x 61, 41 x 31: the last leaves only the row cy = 15
                "stride": (96, 64, 3)}      # levels 96 x 64, 48 x 32, 24 x 16 (smaller than 31: refuses everything)
N_DEVICE = 257
SIDES = ("left", "right", "top", "bottom")


@functools.lru_cache(maxsize=None)
def device_case(name):
    """image (h, w, 3) u8 (the "stride" one a view into a wider buffer), depth, and N_DEVICE keypoints in a fixed
    shuffled order: xy float32 (n, 2), levels int32 (n), and for the border keypoints `side` / `inside` (which side
    the keypoint probes, -1 = none; whether it is the neighbour one pixel inside)."""
    w, h, depth = DEVICE_CASES[name]
    img = make_frames(1, w, h)[0]
    if name == "stride":
        wide = np.zeros((h, w + 7, 3), dtype=np.uint8)
        wide[:, :w] = img
        img = wide[:, :w]
        assert img.strides[0] == 3 * (w + 7)
    rng = np.random.default_rng(41)
    pts = []      # (x, y, level, side, inside)
    for l, (wl, hl) in enumerate(pyramid_dims(w, h, depth)):
        s = float(1 << l)
        xs_in = [R] if wl < 2 * R + 2 else [R, (R + wl - 1 - R) // 2, wl - 1 - R]
        ys_in = [R] if hl < 2 * R + 2 else [R, (R + hl - 1 - R) // 2, hl - 1 - R]
        for cy in ys_in:      # left / right sides: cx in {14, 15, w - 16, w - 15}
            for cx, side, inside in ((R - 1, 0, 0), (R, 0, 1), (wl - 1 - R, 1, 1), (wl - R, 1, 0)):
                pts.append((cx * s, cy * s, l, side, inside))
        for cx in xs_in:      # top / bottom sides
            for cy, side, inside in ((R - 1, 2, 0), (R, 2, 1), (hl - 1 - R, 3, 1), (hl - R, 3, 0)):
                pts.append((cx * s, cy * s, l, side, inside))
    # coordinates ending in .5 on the level (px = c + 0.5 rounds up to c + 1): across the left and top borders too
    pts += [((R - 1 + 0.5) * 1.0, 40.5, 0, -1, 0), ((R - 2 + 0.5) * 1.0, 40.5, 0, -1, 0), (50.5, R - 1.5, 0, -1, 0),
            ((20 + 0.5) * 2.0, (R - 0.5) * 2.0, 1, -1, 0), (33.5, 27.5, 0, -1, 0)]
    pts += [(np.nan, 40.0, 0, -1, 0), (40.0, np.nan, 1, -1, 0), (np.inf, 40.0, 0, -1, 0), (40.0, -np.inf, 0, -1, 0),
            (-np.inf, np.nan, 2, -1, 0), (3e38, 40.0, 0, -1, 0), (-1e9, 40.0, 0, -1, 0)]
    while len(pts) < N_DEVICE:      # interior points on any level, sub-pixel level-0 coordinates
        l = int(rng.integers(0, depth))
        wl, hl = pyramid_dims(w, h, depth)[l]
        if wl < 2 * R + 1 or hl < 2 * R + 1:
            pts.append((float(rng.uniform(0, w)), float(rng.uniform(0, h)), l, -1, 0))
            continue
        s = float(1 << l)
        pts.append((float(rng.uniform(R, wl - 1 - R)) * s, float(rng.uniform(R, hl - 1 - R)) * s, l, -1, 0))
    assert len(pts) == N_DEVICE
    order = rng.permutation(N_DEVICE)
    a = np.array(pts, dtype=np.float64)[order]
    return SimpleNamespace(name=name, img=img, w=w, h=h, depth=depth, xy=a[:, :2].astype(np.float32),
                           levels=a[:, 2].astype(np.int32), side=a[:, 3].astype(np.int64),
                           inside=a[:, 4].astype(np.int64))


@functools.lru_cache(maxsize=None)
def device_expected(name):
    """The reference on the oracle's pyramid of a device case (the device's pyramid is bit-identical to it:
    tests/test_tracker_gpu.py); the GPU test runs the reference again on the levels it downloads."""
    c = device_case(name)
    return reference(oracle_levels(c.img, c.depth), c.xy, c.levels)


TEXTURE_N = 600


@functools.lru_cache(maxsize=None)
def texture_case():
    """600 seed points, 16 px inside the 640 x 480 texture (frame 0 of make_frames), on levels 0, 1, 2 in turn."""
    img = make_frames(1)[0]
    xy = seed_points(TEXTURE_N, border=float(R + 1))
    levels = (np.arange(TEXTURE_N) % 3).astype(np.int32)
    return SimpleNamespace(img=img, depth=3, xy=xy, levels=levels, pyr=oracle_levels(img, 3))


@functools.lru_cache(maxsize=None)
def texture_expected(all_level0=False):
    c = texture_case()
    return reference(c.pyr, c.xy, None if all_level0 else c.levels)


def rotate_image(grey, deg):
    """grey (h, w) u8 rotated about its centre by deg (bilinear, re-quantised to u8), and the map of pixel positions
    (n, 2) of the original to the rotated image."""
    from scipy import ndimage
    h, w = grey.shape
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    ctr = np.array([(w - 1) / 2.0, (h - 1) / 2.0])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    px, py = xs - ctr[0], ys - ctr[1]
    sx, sy = c * px + s * py + ctr[0], -s * px + c * py + ctr[1]      # inverse map: rotated(x) = grey(R^T (x - c) + c)
    out = ndimage.map_coordinates(grey.astype(np.float64), [sy, sx], order=1, mode="nearest")
    Rm = np.array([[c, -s], [s, c]])
    return np.clip(np.rint(out), 0, 255).astype(np.uint8), lambda p: (np.asarray(p, dtype=np.float64) - ctr) @ Rm.T + ctr


@functools.lru_cache(maxsize=None)
def rotation_match(deg, steer=True):
    """Nearest-neighbour matching between frame 0 and its rotation by deg on oracle pyramids (level 0) at ground-truth
    positions: (share of keypoints whose nearest rotated descriptor is their own, keypoints used, mean distance of
    true pairs, mean distance of the best wrong candidate)."""
    c = texture_case()
    grey = c.img[:, :, 0]
    rot, fwd = rotate_image(grey, deg)
    lv_rot = oracle_levels(np.repeat(rot[:, :, None], 3, axis=2), 1)[0]
    xy_rot = fwd(c.xy).astype(np.float32)
    a = reference_level(c.pyr[0], c.xy, 0, steer)
    b = reference_level(lv_rot, xy_rot, 0, steer)
    keep = np.flatnonzero((a["status"] == 0) & (b["status"] == 0))
    d = hamming(a["desc"][keep], b["desc"][keep])
    best = d.argmin(1)
    own = d[np.arange(len(keep)), np.arange(len(keep))]
    wrong = d + np.where(np.eye(len(keep), dtype=bool), 1000, 0)
    return float((best == np.arange(len(keep))).mean()), len(keep), float(own.mean()), float(wrong.min(1).mean())
