"""The reduced-camera solve (k_S_reduce -> k_chol_tiles / k_cholesky_window / k_cholesky_global) at every size,
band width and kernel the host planner can choose, through BundleAdjuster.load / solve / info against oracle.solve
(ba_shape_cases.py has the cases and the bounds; test_ba_shapes_reference_bounds.py shows the reference alone keeps
within half of them).

  size sweep   n = 6 .. 288: every tile-row count NT = 1 .. 18 and every padding 16 NT - n of the last tile, the
               one-workgroup factorisation up to NT = 12 and the dissected band from kSplitMinNT = 13.
  band sweep   NT = 14 and 18 with bands of 2 .. 8 tiles, so separators of every size 1 .. 7 (the suite's other
               split shapes all have 5 or 7), and of 9 and 11 tiles on k_cholesky_global without free intrinsics.
  path sweep   k_cholesky_window (SG_CHOL_WINDOW=1: the fallback when k_chol_tiles is refused) and both instances of
               k_cholesky_global, on the same problems.

What a sweep covers is asserted from info(), so a retuned constant cannot quietly empty it; exact (nd, ns) pairs are
tests/native/ba_plan_check.cpp's business and are not pinned here."""
import os

import numpy as np
import pytest

import ba_shape_cases as bc
from slamgpu import ba

pytestmark = pytest.mark.gpu

TILED, GLOBAL_STAGED = 0, 2
SIZE_CHUNKS = [bc.SIZE_SWEEP[i:i + 8] for i in range(0, len(bc.SIZE_SWEEP), 8)]
PATH_CHUNKS = {
    "window_small": [c for c in bc.PATH_SWEEP if c[3] == bc.PATH_WINDOW and c[0] < 35],
    "window_split_sizes": [c for c in bc.PATH_SWEEP if c[3] == bc.PATH_WINDOW and c[0] >= 35],
    "global_staged": [c for c in bc.PATH_SWEEP if c[3] == bc.PATH_STAGED],
    "global_unstaged": [c for c in bc.PATH_SWEEP if c[3] == bc.PATH_UNSTAGED],
}


def _set_knobs(monkeypatch, env):
    """Every switch of the Cholesky choice and of the iteration chain cleared, then env: set before the handle is
    created, where the run knobs are read."""
    for k in list(os.environ):
        if k.startswith("SG_CHOL_") or k in ("SG_XCHG_MERGE", "SG_SPEC", "SG_LIN_WAVES"):
            monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _load(monkeypatch, solve, r, env):
    _set_knobs(monkeypatch, env)
    p = bc.problem(solve, r)
    g = ba.BundleAdjuster()
    g.load(p)
    return g, p, g.info()


def _solve(monkeypatch, solve, r, env=None):
    """(summary, solved ProblemArrays, info() after the solve: cholesky_stile is what the last iteration did)."""
    g, p, _ = _load(monkeypatch, solve, r, env or {})
    s = g.solve(bc.options())
    info = g.info()
    g.close()
    return s, p, info


def _info(monkeypatch, solve, r, env=None):
    g, _, info = _load(monkeypatch, solve, r, env or {})
    g.close()
    return info


def _name(solve, r, env=None):
    return "solve=%d r=%d%s" % (solve, r, "".join(" %s=%s" % kv for kv in sorted((env or {}).items())))


def _check_size_plan(solve, info, solved=False):
    """n, the path and the split of a size-sweep case: one workgroup below kSplitMinNT = 13 tile rows, two from it."""
    nt = bc.tile_rows(info["n"])
    assert info["n"] == 6 * solve and info["cholesky_path"] == TILED, info
    assert not solved or info["cholesky_stile"] == 1, info
    if nt <= 12:
        assert info["cholesky_split"] == 0, info
    else:
        assert info["cholesky_split"] >= 2, info
        assert 1 <= info["cholesky_separator"] <= 7, info
        assert nt - info["cholesky_split"] - info["cholesky_separator"] >= 1, info


def _against_oracle(oracle_lib, label, sweep, solved):
    """solved: [(name, solve, r, summary, ProblemArrays)]."""
    rows = []
    for name, solve, r, s, p in solved:
        rs, rp = bc.oracle_result(oracle_lib, solve, r)
        assert s["sync_timeouts"] == 0, (name, s)
        rows.append((name, s, p, rs, rp))
    bc.compare(label, sweep, rows)


@pytest.mark.parametrize("chunk", range(len(SIZE_CHUNKS)), ids=lambda i: "solve_%d_%d" % (SIZE_CHUNKS[i][0][0],
                                                                                         SIZE_CHUNKS[i][-1][0]))
def test_size_sweep_matches_oracle(gpu_lib, oracle_lib, monkeypatch, chunk):
    solved = []
    for solve, r in SIZE_CHUNKS[chunk]:
        s, p, info = _solve(monkeypatch, solve, r)
        _check_size_plan(solve, info, solved=True)
        solved.append((_name(solve, r), solve, r, s, p))
    _against_oracle(oracle_lib, "size sweep, solve = %d .. %d" % (SIZE_CHUNKS[chunk][0][0], SIZE_CHUNKS[chunk][-1][0]),
                    "size sweep", solved)


def test_size_sweep_covers_every_tile_row_count_and_padding(gpu_lib, monkeypatch):
    infos = {solve: _info(monkeypatch, solve, r) for solve, r in bc.SIZE_SWEEP}
    for solve, info in infos.items():
        _check_size_plan(solve, info)
    nts = {bc.tile_rows(i["n"]) for i in infos.values()}
    pads = {16 * bc.tile_rows(i["n"]) - i["n"] for i in infos.values()}
    one = {bc.tile_rows(i["n"]) for i in infos.values() if i["cholesky_split"] == 0}
    two = {bc.tile_rows(i["n"]) for i in infos.values() if i["cholesky_split"] >= 2}
    print("size sweep: tile rows %s; paddings %s; one workgroup at NT %s; two at NT %s; band tiles %s" % (
        sorted(nts), sorted(pads), sorted(one), sorted(two), sorted({i["band_tiles"] for i in infos.values()})))
    assert nts == set(range(1, 19))
    assert pads == set(range(0, 16, 2))
    assert one == set(range(1, 13)) and two == set(range(13, 19))


@pytest.mark.parametrize("solve", [35, 46])
def test_band_sweep_matches_oracle(gpu_lib, oracle_lib, monkeypatch, solve):
    solved = []
    for s_, r in bc.BAND_SWEEP:
        if s_ != solve:
            continue
        s, p, info = _solve(monkeypatch, solve, r)
        assert info["n"] == 6 * solve, info
        assert info["cholesky_path"] == (TILED if info["band_tiles"] <= 8 else GLOBAL_STAGED), info
        solved.append((_name(solve, r), solve, r, s, p))
    _against_oracle(oracle_lib, "band sweep, solve = %d" % solve, "band sweep", solved)


def test_band_sweep_covers_every_separator_and_both_sides_of_the_band_limit(gpu_lib, monkeypatch):
    infos = {c: _info(monkeypatch, *c) for c in bc.BAND_SWEEP}
    tiled = {c: i for c, i in infos.items() if i["cholesky_path"] == TILED}
    other = {c: i for c, i in infos.items() if i["cholesky_path"] != TILED}
    seps = {i["cholesky_separator"] for i in tiled.values() if i["cholesky_split"] >= 2}
    print("band sweep: (solve, r) -> band tiles / separator / bottom rows: %s; global: %s" % (
        {c: (i["band_tiles"], i["cholesky_separator"], i["cholesky_split"]) for c, i in tiled.items()},
        {c: (i["band_tiles"], i["cholesky"]) for c, i in other.items()}))
    assert set(tiled) == set(bc.BAND_SPLIT)
    for c, i in tiled.items():
        nt = bc.tile_rows(i["n"])
        assert i["cholesky_split"] >= 2, (c, i)
        assert i["band_tiles"] <= 8 and i["cholesky_separator"] <= i["band_tiles"] - 1, (c, i)
        assert nt - i["cholesky_split"] - i["cholesky_separator"] >= 1, (c, i)
    assert seps == set(range(1, 8))
    assert {i["band_tiles"] for i in tiled.values()} == set(range(2, 9))
    assert all(i["cholesky_path"] == GLOBAL_STAGED and i["band_tiles"] >= 9 for i in other.values()), other
    assert 9 in {i["band_tiles"] for i in other.values()}


@pytest.mark.parametrize("chunk", list(PATH_CHUNKS))
def test_path_sweep_matches_oracle(gpu_lib, oracle_lib, monkeypatch, chunk):
    solved = []
    for solve, r, env, path in PATH_CHUNKS[chunk]:
        s, p, info = _solve(monkeypatch, solve, r, env)
        assert info["n"] == 6 * solve and info["cholesky_path"] == path, (_name(solve, r, env), info)
        assert info["cholesky_split"] == 0, info
        if path != bc.PATH_WINDOW:
            assert info["band_tiles"] > 8, info   # past the window's 128 columns
        solved.append((_name(solve, r, env), solve, r, s, p))
    _against_oracle(oracle_lib, "path sweep, %s" % chunk, "path sweep", solved)


def test_path_sweep_names_the_kernels(gpu_lib, monkeypatch):
    names = {path: _info(monkeypatch, solve, r, env)["cholesky"] for solve, r, env, path in bc.PATH_SWEEP}
    print("path sweep: %s" % names)
    assert names[bc.PATH_WINDOW].startswith("LDS window")
    assert names[bc.PATH_STAGED].startswith("global memory") and "staged" in names[bc.PATH_STAGED]
    assert names[bc.PATH_UNSTAGED].startswith("global memory") and "unstaged" in names[bc.PATH_UNSTAGED]


@pytest.mark.parametrize("solve,r", bc.BAND_SPLIT)
def test_split_band_loader_and_arrival_order_change_no_bit(gpu_lib, monkeypatch, solve, r):
    """The contracts of test_chol_stile_gpu.py at every separator size: the tile-major copy of the band against the
    loader of row-major S (SG_CHOL_STILE=0), and the separator hand-off in both arrival orders (SG_CHOL_DELAY), all
    bit for bit."""
    s0, p0, i0 = _solve(monkeypatch, solve, r)
    assert i0["cholesky_path"] == TILED and i0["cholesky_split"] >= 2 and i0["cholesky_stile"] == 1, i0
    assert s0["ok"] == 1 and s0["sync_timeouts"] == 0 and s0["num_successful_steps"] == bc.ITERATIONS, s0
    for env in ({"SG_CHOL_STILE": "0"}, {"SG_CHOL_DELAY": "bottom"}, {"SG_CHOL_DELAY": "top"}):
        s1, p1, i1 = _solve(monkeypatch, solve, r, env)
        assert i1["cholesky_stile"] == (0 if "SG_CHOL_STILE" in env else 1), (env, i1)
        assert (i1["cholesky_split"], i1["cholesky_separator"]) == (i0["cholesky_split"], i0["cholesky_separator"])
        assert s1 == s0, (env, s1, s0)
        np.testing.assert_array_equal(p1.q, p0.q)
        np.testing.assert_array_equal(p1.t, p0.t)
        np.testing.assert_array_equal(p1.X, p0.X)
