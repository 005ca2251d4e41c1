"""sg_slam_optimize_pose_graph on the device against the numpy reference (tests/posegraph_cases.py): every scene's
status, termination type and iteration counts equal the reference's, its final cost, poses and log-scales within
MARGIN * SPREAD (the reference's own rounding floor, recomputed by tests/test_posegraph_reference_bounds.py);
reproducibility bit for bit, alone and beside other graphs in either order; a graph without an anchor beside a solved
one; and the loop-closing chain AlignPoints -> PoseEdges(sim) -> OptimizePoseGraph(move_points)."""
import numpy as np
import pytest

import posegraph_cases as pc
from slamgpu.ba import Slam

pytestmark = pytest.mark.gpu


def _solve(names, frames_of=None, slam=None, **kw):
    """One call with the named scenes as graphs on one map (scene i's frames follow scene i - 1's)."""
    scs = [pc.scene(n) for n in names]
    q = np.vstack([s["q"] for s in scs])
    t = np.vstack([s["t"] for s in scs])
    m = pc.frames_map(q, t)
    off = np.cumsum([0] + [len(s["q"]) for s in scs])
    graphs = [pc.graph_of(s, np.arange(off[i], off[i + 1])) for i, s in enumerate(scs)]
    slam = slam or Slam(options=pc.solver_options(names[0]))
    kw.setdefault("range_", scs[0]["range"])
    kw.setdefault("fix_scale", scs[0]["fix_scale"])
    out = slam.OptimizePoseGraph(m, graphs, **kw)
    return m, [pc.states(m, np.arange(off[i], off[i + 1]), out[i]["log_scale"]) for i in range(len(scs))], out, slam


@pytest.mark.parametrize("name", pc.SCENES)
def test_scene_matches_the_reference(name):
    sc, ref = pc.scene(name), pc.reference(name)
    m, (x,), (out,), slam = _solve([name])
    print(name, {k: out[k] for k in ("status", "termination", "num_iterations", "num_successful_steps",
                                     "num_unsuccessful_steps", "num_invalid_steps", "final_cost")})
    d = pc.compare(x, ref["x"])
    d["cost"] = abs(out["final_cost"] - ref["final_cost"])
    print(name, "against the reference:", d, "bounds:", {k: pc.bound(name, k) for k in d})
    assert out["status"] == "OK" and out["ok"] == 1 and out["termination"] == ref["termination"]
    for key in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps"):
        assert out[key] == ref[key], key
    assert abs(out["initial_cost"] - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
    for key, val in d.items():
        assert val <= pc.bound(name, key), (key, val, pc.bound(name, key))
    fixed = np.flatnonzero(sc["fixed"])
    assert (x[fixed, :4] == sc["q"][fixed]).all() and (x[fixed, 4:7] == sc["t"][fixed]).all() and (x[fixed, 7] == 0).all()
    free = np.flatnonzero(sc["fixed"] == 0)
    assert (np.abs(np.linalg.norm(x[free, :4], axis=1) - 1.0) <= 4e-16).all() and (x[free, 3] >= 0).all()
    # the facade's bookkeeping follows the graph that ran
    assert slam.iterations() == out["num_iterations"] and slam.error() == out["final_cost"]
    if name == "ring8":
        xt = np.zeros_like(x)
        xt[:, :4], xt[:, 4:7] = sc["q_true"], sc["t_true"]
        own, got = pc.compare(ref["x"], xt), pc.compare(x, xt)
        print("ring8 against the truth:", got, "the reference:", own)
        for key in got:   # MARGIN times the reference's own error against the truth, never below its rounding floor
            assert got[key] <= pc.MARGIN * max(own[key], pc.SPREAD[name][key]), key
        assert out["final_cost"] < 1e-20
    if name == "rigid12":
        assert (out["log_scale"] == 0.0).all()
    if name == "drift12":
        assert np.ptp(out["log_scale"][1:]) > 0.05 and out["log_scale"][0] == 0.0


def test_badloop12_lands_far_from_the_result_without_a_loss():
    ref = pc.reference("badloop12")
    _, (x,), (out,), _ = _solve(["badloop12"])
    _, (x0,), (out0,), _ = _solve(["badloop12"], range_=0.0)
    near, far = pc.compare(x, ref["x"]), pc.compare(x, x0)
    print("badloop12: from the reference", near, "from the solve without a loss", far, out0["status"])
    assert near["t"] <= pc.bound("badloop12", "t") and near["rot_deg"] <= pc.bound("badloop12", "rot_deg")
    assert far["t"] > 10.0 and far["rot_deg"] > 1.0   # the wrong edge asks for hundreds of map units and a half turn


def test_results_do_not_depend_on_the_position_in_the_call_or_the_run():
    _, (c,), (oc,), slam = _solve(["chords24"])
    _, (d,), (od,), _ = _solve(["drift12"], slam=slam)
    _, (c1, d1), o1, _ = _solve(["chords24", "drift12"], slam=slam)
    _, (d2, c2), o2, _ = _solve(["drift12", "chords24"], slam=slam)
    _, (c3, d3), o3, _ = _solve(["chords24", "drift12"], slam=Slam(options=pc.solver_options("chords24")))
    for got in (c1, c2, c3):
        assert got.tobytes() == c.tobytes()
    for got in (d1, d2, d3):
        assert got.tobytes() == d.tobytes()
    for a, b in ((o1[0], oc), (o2[1], oc), (o3[0], oc), (o1[1], od), (o2[0], od), (o3[1], od)):
        assert a["final_cost"] == b["final_cost"] and a["num_iterations"] == b["num_iterations"]
        assert a["trust_region_radius"] == b["trust_region_radius"] and a["initial_cost"] == b["initial_cost"]


def test_a_graph_without_an_anchor_beside_a_solved_one():
    slam = Slam(options=pc.solver_options("ring8"))
    m, (xa, xb), out, _ = _solve(["two_comp", "ring8"], slam=slam)
    two, ring = pc.scene("two_comp"), pc.scene("ring8")
    assert [o["status"] for o in out] == ["NO_ANCHOR", "OK"]
    assert (xa[:, :4] == two["q"]).all() and (xa[:, 4:7] == two["t"]).all() and (xa[:, 7] == 0).all()
    assert out[0]["termination"] == "DID_NOT_RUN" and out[0]["num_iterations"] == 0
    _, (alone,), _, _ = _solve(["ring8"])
    assert xb.tobytes() == alone.tobytes() and not (xb[1:, 4:7] == ring["t"][1:]).any()
    assert slam.iterations() == out[1]["num_iterations"]


def test_loop_closing_chain_beats_one_rigid_similarity():
    r = pc.loop_reference()
    print("numpy, closing frames: rigid %.4g deg %.4g units; pose graph %.4g deg %.4g units" % (*r["rigid"], *r["graph"]))
    assert 2.0 * r["graph"][0] <= r["rigid"][0] and 2.0 * r["graph"][1] <= r["rigid"][1]
    ls = pc.loop_scene()
    slam = Slam()
    m = ls["map"].copy()
    groups = [ls["groups"][c] for c in pc.LOOP_CLOSING] + [np.vstack([ls["groups"][c] for c in pc.LOOP_CLOSING])]
    al = slam.AlignPoints(m, groups, threshold=pc.LOOP_THRESHOLD)
    assert all(a["solved"] for a in al), [a["status"] for a in al]
    # what the library could do before: the one similarity of all matches, applied to the drifted piece
    rigid = m.copy()
    slam.ApplySimilarity(rigid, al[2]["scale"], al[2]["q"], al[2]["t"], ls["piece_frames"], ls["piece_points"])
    err_rigid = pc.closing_errors(ls, rigid.q, rigid.t)
    # the chain: one loop edge per closing frame from its own similarity, odometry edges from the map as it stands
    loop = np.vstack([slam.PoseEdges(m, [(c, 0)], (al[i]["scale"], al[i]["q"], al[i]["t"]))
                      for i, c in enumerate(pc.LOOP_CLOSING)])
    assert len(slam.CovisiblePairs(m, np.arange(m.num_frames), 30)) >= m.num_frames - 1
    g = pc.loop_graph(ls, slam.PoseEdges(m, ls["odo"]), loop)
    before = m.copy()
    out = slam.OptimizePoseGraph(m, [g], move_points=True)[0]
    err_graph = pc.closing_errors(ls, m.q, m.t)
    print("device, closing frames: rigid %.4g deg %.4g units; pose graph %.4g deg %.4g units; %s after %d iterations" %
          (*err_rigid, *err_graph, out["termination"], out["num_iterations"]))
    assert out["status"] == "OK"
    assert err_graph[0] < err_rigid[0] and err_graph[1] < err_rigid[1]
    assert (m.X != before.X).any() and (m.X.reshape(-1, 4)[:, 3] == before.X.reshape(-1, 4)[:, 3]).all()
    assert (m.q[:8] == before.q[:8]).all() and (m.t[:6] == before.t[:6]).all()     # frames 0 and 1 are fixed
