"""The numpy reference of sg_tracker_detect (include/slamgpu.h) and the cases of its tests.  Test material only:
nothing here is a path of the library.

detect() is the contract written plainly on a list of level arrays: the score of the radius-3 ring as fp32 differences,
mins and maxes, the 3 x 3 suppression, the admissible rectangle, the 32 x 32 cells with the two-threshold rule and the
per-cell ranking, the output order and the cap.  Nothing in it sums or multiplies pixel values, so it has one right
answer and the tests demand exact equality with it.

Cases: CASES maps a name to (image, depth); option_sets(levels) gives the option sets every equality test runs, two
of which (the median threshold and the caps) are derived from the level arrays they are run on."""
import functools
from types import SimpleNamespace

import numpy as np

from describe_cases import oracle_levels, pyramid_dims  # noqa: F401  (re-exported for the tests)
from slamgpu.video import make_frames

CELL = 32
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0),
        (-3, -1), (-2, -2), (-1, -3))
T_LO, T_HI = np.float32(0.01), np.float32(20.0 / 255.0)
DEFAULTS = dict(threshold=T_HI, min_threshold=T_LO, first_level=0, num_levels=0, border=4, per_cell=4, max_keypoints=0)


# ------------------------------------------------------------------------------------------------ the reference
def score_map(img):
    """s (h, w) float32 of level array img; -inf where the ring does not fit (no rule reads it there)."""
    img = np.asarray(img, dtype=np.float32)
    h, w = img.shape
    s = np.full((h, w), -np.inf, dtype=np.float32)
    if h < 7 or w < 7:
        return s
    c = img[3:h - 3, 3:w - 3]
    d = np.stack([img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING])      # fp32 subtractions
    assert d.dtype == np.float32
    dd = np.concatenate([d, d[:8]])
    bright = np.max([dd[k:k + 9].min(axis=0) for k in range(16)], axis=0)
    dark = np.max([(-dd[k:k + 9]).min(axis=0) for k in range(16)], axis=0)
    s[3:h - 3, 3:w - 3] = np.maximum(bright, dark)
    return s


def candidates(img, t_lo, border):
    """(x, y, s) of the candidates of a level in row-major order."""
    assert border >= 4
    h, w = img.shape
    if w - 1 - border < border or h - 1 - border < border:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    s = score_map(img)
    ys, xs = np.mgrid[border:h - border, border:w - border]
    p = s[ys, xs]
    ok = p > np.float32(t_lo)
    for dx, dy in ((-1, -1), (0, -1), (1, -1), (-1, 0)):      # earlier in row-major order: strictly greater
        ok &= p > s[ys + dy, xs + dx]
    for dx, dy in ((1, 0), (-1, 1), (0, 1), (1, 1)):          # later: greater or equal
        ok &= p >= s[ys + dy, xs + dx]
    return xs[ok], ys[ok], p[ok]


def detect_level(img, t_lo, t_hi, border, per_cell):
    """One level: dict of the kept keypoints x, y, s (cell row-major, then rank), and the level's cells, candidates,
    low_cells; `cand` keeps the candidates and `cell_info` per cell (candidates, eligible, best score) for the bounds
    test."""
    img = np.asarray(img, dtype=np.float32)
    h, w = img.shape
    cx, cy = (w + CELL - 1) // CELL, (h + CELL - 1) // CELL
    x, y, s = candidates(img, t_lo, border)
    cell = (y // CELL) * cx + x // CELL
    kx, ky, ks, low, info = [], [], [], 0, {}
    for c in np.unique(cell):
        m = np.flatnonzero(cell == c)
        hi = s[m] > np.float32(t_hi)
        if hi.any():
            m = m[hi]
        else:
            low += 1
        order = np.lexsort((y[m] * w + x[m], -s[m].astype(np.float64)))      # s descending, pixel index ascending
        info[int(c)] = (int((cell == c).sum()), len(m), float(s[m].max()))
        m = m[order][:per_cell]
        kx += list(x[m])
        ky += list(y[m])
        ks += list(s[m])
    return dict(x=np.array(kx, np.int64), y=np.array(ky, np.int64), s=np.array(ks, np.float32), w=w, h=h,
                cells=cx * cy, candidates=len(x), low_cells=low, cand=(x, y, s), cell_info=info)


def detect(levels_img, **options):
    """The contract on a pyramid (list of level arrays): SimpleNamespace of xy float32 (n, 2), levels int32, score
    float32, per_level (list of dicts as sg_detect_level), and `by_level`, detect_level's records."""
    o = dict(DEFAULTS, **options)
    depth = len(levels_img)
    first = o["first_level"]
    last = depth if o["num_levels"] == 0 else first + o["num_levels"]
    assert 0 <= first < depth and first < last <= depth and 0 <= o["min_threshold"] <= o["threshold"]
    per_level = [dict(width=a.shape[1], height=a.shape[0], cells=0, candidates=0, low_cells=0, keypoints=0)
                 for a in levels_img]
    by_level = {}
    X, Y, S, L = [], [], [], []
    for l in range(first, last):
        r = detect_level(levels_img[l], o["min_threshold"], o["threshold"], o["border"], o["per_cell"])
        by_level[l] = r
        per_level[l].update(cells=r["cells"], candidates=r["candidates"], low_cells=r["low_cells"])
        X.append(r["x"])
        Y.append(r["y"])
        S.append(r["s"])
        L.append(np.full(len(r["x"]), l, np.int64))
    X, Y, S, L = (np.concatenate(v) for v in (X, Y, S, L))
    cap = o["max_keypoints"]
    if cap > 0 and len(X) > cap:
        w = np.array([levels_img[l].shape[1] for l in L], dtype=np.int64)
        order = np.lexsort((Y * w + X, L, -S.astype(np.float64)))      # s descending, level, pixel index ascending
        keep = np.zeros(len(X), dtype=bool)
        keep[order[:cap]] = True
        X, Y, S, L = X[keep], Y[keep], S[keep], L[keep]
    for l in range(first, last):
        per_level[l]["keypoints"] = int((L == l).sum())
    scale = (2.0 ** L).astype(np.float32)
    xy = np.stack([X.astype(np.float32) * scale, Y.astype(np.float32) * scale], 1).reshape(-1, 2)
    return SimpleNamespace(xy=xy, levels=L.astype(np.int32), score=S.astype(np.float32), per_level=per_level,
                           by_level=by_level, x=X, y=Y)


# ------------------------------------------------------------------------------------------------ cases
def _rgb(grey):
    return np.repeat(np.ascontiguousarray(grey, dtype=np.uint8)[:, :, None], 3, axis=2)


PLANT_W, PLANT_H = 97, 70
# (x, y, value) of the 3 x 3 squares' centres on the flat field of 128
PLANTED = (
    (31, 10, 255), (32, 21, 0), (63, 10, 0), (64, 21, 255),            # astride the cell columns 31 | 32, 63 | 64
    (12, 31, 255), (47, 32, 0), (20, 63, 255), (40, 64, 0),            # astride the cell rows 31 | 32, 63 | 64
    (31, 31, 255), (64, 32, 0),                                        # the last pixel of a cell, the first of one
    (40, 46, 255), (54, 46, 255),                                      # two equal squares in cell (1, 1): a tie
    (15, 15, 0), (81, 54, 255),                                        # exactly border 15 from two sides each
    (14, 46, 0), (82, 40, 0), (47, 14, 255), (66, 55, 0),              # one pixel further out than border 15
    (4, 4, 255), (92, 65, 0),                                          # exactly border 4 from two sides each
    (3, 58, 255), (93, 8, 0), (80, 3, 255), (80, 66, 0))               # one pixel further out than border 4
STRADDLED = (("x", 31, 32), ("x", 63, 64), ("y", 31, 32), ("y", 63, 64))


def planted_image():
    g = np.full((PLANT_H, PLANT_W), 128, dtype=np.uint8)
    for x, y, v in PLANTED:
        g[y - 1:y + 2, x - 1:x + 2] = v
    return _rgb(g)


def _strided(img, pad=7):
    h, w = img.shape[:2]
    wide = np.zeros((h, w + pad, 3), dtype=np.uint8)
    wide[:, :w] = img
    view = wide[:, :w]
    assert view.strides[0] == 3 * (w + pad)
    return view


@functools.lru_cache(maxsize=None)
def case(name):
    """SimpleNamespace(name, img (h, w, 3) u8, w, h, depth)."""
    if name == "odd":            # levels 161 x 121, 81 x 61, 41 x 31: partial last cells, several cells per level
        img, depth = make_frames(1, 161, 121)[0], 3
    elif name == "stride":       # levels 96 x 64, 48 x 32, 24 x 16, the image a view with a padded row stride
        img, depth = _strided(make_frames(1, 96, 64)[0]), 3
    elif name == "planted":      # levels 97 x 70, 49 x 35
        img, depth = planted_image(), 2
    elif name == "constant":     # no keypoints
        img, depth = _rgb(np.full((48, 64), 93)), 2
    elif name == "thin":         # 33 x 9: with border 4 one admissible row and an empty second cell column; 17 x 5
        img, depth = make_frames(1, 33, 9)[0], 2
    else:
        raise KeyError(name)
    return SimpleNamespace(name=name, img=img, w=img.shape[1], h=img.shape[0], depth=depth)


CASES = ("odd", "stride", "planted", "constant", "thin")
TEXTURE_CASES = ("odd", "stride")


@functools.lru_cache(maxsize=None)
def case_levels(name):
    """The oracle's pyramid of a case (the device's is bit-identical to it: tests/test_tracker_gpu.py)."""
    c = case(name)
    return oracle_levels(c.img, c.depth)


def median_threshold(levels_img, border=4):
    """The median over the level-0 cells that hold candidates of the cell's best score (T_LO, `border`): as t_hi it
    puts about half of those cells on each branch of the two-threshold rule.  T_HI when level 0 has no candidate."""
    r = detect_level(levels_img[0], T_LO, np.float32(np.inf), border, 1)
    best = sorted(v[2] for v in r["cell_info"].values())
    return np.float32(best[len(best) // 2]) if best else T_HI


def option_sets(levels_img):
    """name -> options (over DEFAULTS) of every equality test, for the pyramid they are run on."""
    depth = len(levels_img)
    total = len(detect(levels_img).xy)
    sets = {
        "border4": dict(),
        "border15": dict(border=15),
        "per_cell1_equal_thresholds": dict(per_cell=1, threshold=T_LO),
        "per_cell2": dict(per_cell=2, border=15),
        "per_cell16": dict(per_cell=16),
        "median": dict(threshold=median_threshold(levels_img)),
        "level1": dict(first_level=1, num_levels=1),
        "cap_half": dict(max_keypoints=max(1, total // 2)),
        "cap_equal": dict(max_keypoints=max(1, total)),
    }
    if depth >= 3:
        sets["levels12"] = dict(first_level=1, num_levels=2, border=15)
    return sets
