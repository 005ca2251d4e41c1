"""The separator hand-off of the dissected band Cholesky (k_chol_tiles): the bottom workgroup
publishes its W tiles, z', failure slots and separator contribution write-through and signals once; the top
workgroup's separator waves poll and read the contribution with the matching loads.  Against the one-workgroup
factorisation the dissected solve is checked by test_ba_gpu.py::test_dissected_band_matches_one_workgroup."""
import numpy as np
import pytest

from slamgpu import ba
from slamgpu.capi import default_solver_options
from slamgpu.scene import make_config, make_scene

pytestmark = pytest.mark.gpu


def _problem(frames, points):
    if points is None:
        m = make_config("C2")
    else:
        m = make_scene(num_frames=frames, num_points=points, seed=5, run_max=14)
    return ba.problem_from_map_frames(m, m.num_frames - 2, m.num_frames, 2.0)


def _solve(pa, monkeypatch, env):
    monkeypatch.delenv("SG_CHOL_DELAY", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = pa.copy()
    g = ba.BundleAdjuster()
    g.load(p)
    info = g.info()
    s = g.solve(default_solver_options(max_num_iterations=8))
    g.close()
    return s, p, info


@pytest.mark.parametrize("frames,points", [(36, 8000), (50, None)])
def test_arrival_order_does_not_change_a_bit(gpu_lib, monkeypatch, frames, points):
    """Both arrival orders of the hand-off give the plain solve bit for bit: SG_CHOL_DELAY=bottom keeps the top
    workgroup's separator waves spinning on a late producer, SG_CHOL_DELAY=top has the flag set before they look.
    A stale separator tile, W tile or z' shows up as a different solve."""
    pa = _problem(frames, points)
    s0, p0, info = _solve(pa, monkeypatch, {})
    assert info["cholesky_split"] >= 2
    assert s0["ok"] == 1 and s0["sync_timeouts"] == 0
    for who in ("bottom", "top"):
        s1, p1, _ = _solve(pa, monkeypatch, {"SG_CHOL_DELAY": who})
        assert s1["sync_timeouts"] == 0
        assert s1 == s0
        np.testing.assert_array_equal(p0.q, p1.q)
        np.testing.assert_array_equal(p0.t, p1.t)
        np.testing.assert_array_equal(p0.X, p1.X)
