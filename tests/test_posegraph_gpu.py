"""sg_slam_optimize_pose_graph on the device against the numpy reference (tests/posegraph_cases.py): every scene's
status, termination type and iteration counts equal the reference's, its final cost, poses and log-scales within
MARGIN * SPREAD (the reference's own rounding floor, recomputed by tests/test_posegraph_reference_bounds.py);
reproducibility bit for bit, alone and beside other graphs in either order; a graph without an anchor beside a solved
one; the paths off the converging one (rejected steps, invalid steps up to SG_PG_FAILED, NO_CONVERGENCE, the radius
test; PATH_SCENES and the far scenes), alone and beside solved graphs in one launch; a graph at the node cap behind
another one, against the committed reference result; and the loop-closing chain AlignPoints -> PoseEdges(sim) ->
OptimizePoseGraph(move_points)."""
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
    print(name, "the reference:", {k: ref[k] for k in ("termination", "num_iterations", "num_successful_steps",
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
    if name in ("rigid12", "farrigid12"):
        assert (out["log_scale"] == 0.0).all()
    if name in ("far12", "farrigid12", "farcauchy12"):   # rejected steps: the solve goes on from the kept state
        assert out["num_unsuccessful_steps"] >= (1 if name == "farcauchy12" else 3)
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


COUNTS = ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps")


@pytest.mark.parametrize("name", pc.PATH_SCENES)
def test_paths_that_do_not_end_converged(name):
    """Invalid steps up to NUMERICAL_FAILURE (the pivot that is exactly 0 in the first, a middle and the last column),
    NO_CONVERGENCE at max_num_iterations, and rejected steps down to min_trust_region_radius: status, termination and
    all four counts equal the reference's, and the map is left as the contract says."""
    sc, ref = pc.scene(name), pc.reference(name)
    slam = Slam(options=pc.solver_options(name))
    prev = None
    for _ in range(2):   # the second call reuses the handle's workspace after a failed graph
        m = pc.frames_map(sc["q"], sc["t"])
        before, it0 = m.copy(), slam.iterations()
        out = slam.OptimizePoseGraph(m, [pc.graph_of(sc)], range_=sc["range"], fix_scale=sc["fix_scale"])[0]
        pc.check_path_result(name, out, m, before)
        assert slam.iterations() - it0 == ref["num_iterations"]
        last = slam.last_summary()
        print(name, "sg_slam_last_summary:", {k: last[k] for k in ("ok", "termination") + COUNTS})
        assert last["ok"] == ref["ok"] and last["termination"] == ref["termination"]
        for key in COUNTS:
            assert last[key] == ref[key], key
        if prev is not None:
            assert out["final_cost"] == prev[0]["final_cost"]
            assert out["trust_region_radius"] == prev[0]["trust_region_radius"]
            assert m.q.tobytes() == prev[1].q.tobytes() and m.t.tobytes() == prev[1].t.tobytes()
        prev = (out, m)


def test_failed_and_rejecting_graphs_beside_solved_ones():
    """One launch holds graphs that reject steps, fail on invalid steps, have no anchor and solve at once, in both
    orders: each workgroup's control flow is its own.  Every graph runs with min_lm_diagonal = 0, which the loose
    scenes need and which changes nothing for the others (tests/test_posegraph_reference_bounds.py)."""
    from slamgpu.capi import default_solver_options
    names = ["far12", "loose9", "two_comp", "complete48", "loose_last9", "ring8"]
    want = dict(zip(names, ["OK", "FAILED", "NO_ANCHOR", "OK", "FAILED", "OK"]))
    opt = lambda: default_solver_options(min_lm_diagonal=0.0)
    alone = {}
    for n in names:
        if want[n] == "OK":
            _, (x,), (o,), _ = _solve([n], slam=Slam(options=opt()))
            alone[n] = (x, o)
    far, ref = alone["far12"][1], pc.reference("far12")
    print("far12 alone with min_lm_diagonal = 0:", {k: far[k] for k in COUNTS}, "the reference:", {k: ref[k] for k in COUNTS})
    assert far["num_unsuccessful_steps"] >= 3 and all(far[k] == ref[k] for k in COUNTS)
    slam = Slam(options=opt())
    for order in (names, names[::-1]):
        it0 = slam.iterations()
        _, xs, out, _ = _solve(order, slam=slam)
        print([(n, o["status"], o["termination"], o["num_iterations"], o["num_unsuccessful_steps"], o["num_invalid_steps"])
               for n, o in zip(order, out)])
        assert [o["status"] for o in out] == [want[n] for n in order]
        for n, x, o in zip(order, xs, out):
            sc = pc.scene(n)
            if want[n] == "OK":
                x1, o1 = alone[n]
                assert x.tobytes() == x1.tobytes(), n
                for key in ("final_cost", "initial_cost", "trust_region_radius", "termination") + COUNTS:
                    assert o[key] == o1[key], (n, key)
            else:
                assert (x[:, :4] == sc["q"]).all() and (x[:, 4:7] == sc["t"]).all() and (x[:, 7] == 0).all(), n
            if want[n] == "FAILED":
                assert o["ok"] == 0 and o["termination"] == "NUMERICAL_FAILURE"
                assert (o["num_invalid_steps"], o["num_unsuccessful_steps"], o["num_successful_steps"]) == (5, 4, 0)
            if want[n] == "NO_ANCHOR":
                assert o["termination"] == "DID_NOT_RUN" and o["num_iterations"] == 0
        # the facade counts the graphs that ran, failed ones included, and keeps the last of them
        assert slam.iterations() - it0 == sum(o["num_iterations"] for o in out)
        last = [o for o in out if o["termination"] != "DID_NOT_RUN"][-1]
        assert slam.last_summary()["num_iterations"] == last["num_iterations"] and slam.error() == last["final_cost"]


def test_cap1024_behind_another_graph():
    """A graph at the node cap (kPgMaxNodes) in the second place of a call, behind complete48: node0 = 48, col0 = 47,
    1128 edges and 1128 blocks of L ahead of its own."""
    _, (xc, x), (oc, out), _ = _solve(["complete48", "cap1024"])
    assert oc["status"] == "OK" and oc["num_iterations"] == pc.reference("complete48")["num_iterations"]
    d = pc.compare(xc, pc.reference("complete48")["x"])
    assert all(d[k] <= pc.bound("complete48", k) for k in d), d
    pc.check_cap1024(x, out)


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
