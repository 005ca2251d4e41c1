"""The tile-major copy of S's band (St): k_S_reduce writes every band tile a second time, in the order
and register layout k_chol_tiles consumes it (the bottom workgroup's tiles already reversed and transposed, the
padding past n baked in), and k_chol_tiles loads its tiles from there.  Pure data movement: against the loader of
row-major S (SG_CHOL_STILE=0) every solve must come out bit for bit.  The slots themselves are checked on the host by
test_stile_plan.py."""
import numpy as np
import pytest

from slamgpu import ba
from slamgpu.capi import default_solver_options
from slamgpu.scene import make_config, make_scene

pytestmark = pytest.mark.gpu

# frames, points -> tile rows of S (n = 6 (frames - 2)), what the shape exercises
SHAPES = {
    "nt13_split_padded": (36, 8000),   # n = 204: 13 tile rows, two workgroups, the last tile padded by 4 rows
    "nt15_split": (42, 8000),          # n = 240: 15 tile rows, two workgroups, no padding
    "nt7_one_workgroup": (20, 4000),   # n = 108: 7 tile rows, one workgroup (the top loader only), padded by 4
}


def _problem(frames, points):
    m = make_scene(num_frames=frames, num_points=points, seed=5, run_max=14)
    return ba.problem_from_map_frames(m, m.num_frames - 2, m.num_frames, 2.0)


def _solve(pa, monkeypatch, env, options=None):
    for k in ("SG_CHOL_STILE", "SG_CHOL_DELAY", "SG_XCHG_MERGE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = pa.copy()
    g = ba.BundleAdjuster()
    g.load(p)
    s = g.solve(options or default_solver_options(max_num_iterations=8))
    info = g.info()
    g.close()
    return s, p, info


def _assert_same_bits(a, b):
    (s0, p0, _), (s1, p1, _) = a, b
    assert s1 == s0
    np.testing.assert_array_equal(p0.q, p1.q)
    np.testing.assert_array_equal(p0.t, p1.t)
    np.testing.assert_array_equal(p0.X, p1.X)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tile_major_band_does_not_change_a_bit(gpu_lib, monkeypatch, shape):
    """SG_CHOL_STILE=0 against the default, and on the split shapes the default again in both arrival orders of the
    separator hand-off (SG_CHOL_DELAY).  A tile in the wrong slot, a transposed element or a missing identity in
    the padding shows up as a different (or failed) solve."""
    frames, points = SHAPES[shape]
    pa = _problem(frames, points)
    nt = (6 * (frames - 2) + 15) // 16
    old = _solve(pa, monkeypatch, {"SG_CHOL_STILE": "0"})
    new = _solve(pa, monkeypatch, {})
    for _, _, info in (old, new):
        assert info["cholesky"].startswith("tiled band") and info["n"] == 6 * (frames - 2)
        if shape == "nt7_one_workgroup":
            assert nt == 7 and info["cholesky_split"] == 0
        else:
            assert nt == (13 if shape == "nt13_split_padded" else 15)
            assert info["cholesky_split"] >= 2 and nt - info["cholesky_split"] - info["cholesky_separator"] >= 1
    assert old[2]["cholesky_stile"] == 0 and new[2]["cholesky_stile"] == 1
    assert old[0]["ok"] == 1 and old[0]["sync_timeouts"] == 0 and old[0]["num_iterations"] >= 2
    _assert_same_bits(old, new)
    if shape != "nt7_one_workgroup":
        for who in ("bottom", "top"):
            late = _solve(pa, monkeypatch, {"SG_CHOL_DELAY": who})
            assert late[2]["cholesky_stile"] == 1
            _assert_same_bits(old, late)


def test_merged_exchange_keeps_the_row_major_loader(gpu_lib, monkeypatch):
    """Where k_S_reduce is not the last writer of S (the landmark shards' merged exchange chain, forced on one rank by
    SG_XCHG_MERGE=force: the damping is added after the exchange) St would be stale, so k_chol_tiles keeps the loader
    of row-major S.  The solve matches the default chain as test_ba_gpu.py::test_merged_exchange_chain_on_one_rank
    asks (same steps, cost 1e-12 relative, rotations 1e-10, translations 1e-6 mm)."""
    m = make_config("C2")
    pa = ba.problem_from_map_frames(m, 48, 50, 2.0)
    o = default_solver_options()
    s0, p0, i0 = _solve(pa, monkeypatch, {}, o)
    s1, p1, i1 = _solve(pa, monkeypatch, {"SG_XCHG_MERGE": "force"}, o)
    assert i0["cholesky_stile"] == 1 and i1["cholesky_stile"] == 0
    assert i0["cholesky_split"] == i1["cholesky_split"] >= 2
    assert s1["ok"] == 1 and s1["sync_timeouts"] == 0
    assert s0["num_iterations"] == s1["num_iterations"]
    assert s0["num_successful_steps"] == s1["num_successful_steps"]
    assert abs(s0["final_cost"] - s1["final_cost"]) <= 1e-12 * s0["final_cost"]
    np.testing.assert_allclose(p1.q, p0.q, rtol=0, atol=1e-10)
    np.testing.assert_allclose(p1.t, p0.t, rtol=0, atol=1e-6)
