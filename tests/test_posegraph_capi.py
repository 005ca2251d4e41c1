"""Argument handling of sg_slam_optimize_pose_graph, its statuses that are decided on the host, and the host-only calls
around it (sg_map_pose_edges, sg_map_covisible_pairs, the move_points step): needs the library but no GPU.  Every
argument error is found by the host-only planner before the device is touched, so an opaque dummy handle is enough.
The planner's CPU executor (sg_posegraph_debug_cpu_solve, the same plan and arithmetic the kernel follows) is held to
the numpy reference on every scene here, the scenes that end failed, unconverged or by the radius test (PATH_SCENES)
and the graph at the node cap included, so that a fault of the plan or the arithmetic shows without a device."""
import ctypes as C

import numpy as np
import pytest

import posegraph_cases as pc
from slamgpu.capi import PG_STATUS, SgPosegraphOptions, SgSolverSummary, load_library
from slamgpu.scene import make_config, project_np, quat_to_matrix

IP, DP = C.POINTER(C.c_int32), C.POINTER(C.c_double)
MAP_ARRAYS = ("k", "q", "t", "X", "point_flags", "point_uncertainty", "obs_pt", "obs_frame", "obs_point",
              "obs_disabled", "obs_error", "frame_camera", "frame_prev")


def _arrays(m):
    return {n: getattr(m, n).tobytes() for n in MAP_ARRAYS}


def test_symbols_defaults_and_struct_sizes():
    lib = load_library()
    assert lib.sg_slam_optimize_pose_graph and lib.sg_map_pose_edges and lib.sg_map_covisible_pairs
    o = SgPosegraphOptions(range=7.0, fix_scale=7, move_points=7)
    lib.sg_posegraph_options_default(C.byref(o))
    assert (o.range, o.fix_scale, o.move_points) == (0.0, 0, 0)
    assert C.sizeof(SgPosegraphOptions) == 16
    assert PG_STATUS == {0: "OK", 1: "DID_NOT_RUN", 2: "NO_ANCHOR", 3: "FAILED"}


class _Call:
    """One graph (ring8) as raw arrays, with outputs that show any write."""

    def __init__(self, name="ring8"):
        sc = pc.scene(name)
        self.m = pc.frames_map(sc["q"], sc["t"])
        self.fr = np.arange(len(sc["q"]), dtype=np.int32)
        self.fx = sc["fixed"].astype(np.int32).copy()
        self.ab = sc["edges"].astype(np.int32).reshape(-1).copy()
        self.meas = sc["meas"].reshape(-1).copy()
        self.w = sc["weights"].reshape(-1).copy()
        self.noff = np.array([0, len(self.fr)], dtype=np.int32)
        self.eoff = np.array([0, len(sc["edges"])], dtype=np.int32)
        self.n = 1
        self.o = SgPosegraphOptions(range=0.0, fix_scale=0, move_points=0)
        self.status = np.full(4, 77, dtype=np.int32)
        self.ls = np.full(64, 7.5)
        self.sums = (SgSolverSummary * 4)()
        self.sums[0].num_iterations = 77
        self.buf = C.create_string_buffer(64)
        self.handle = C.cast(self.buf, C.c_void_p)   # an opaque non-null handle: it must never be touched
        self.raw = bytes(self.buf.raw)
        self.before = _arrays(self.m)
        self.null = set()

    def run(self, lib):
        ms = self.m.struct()
        a = lambda name, arr, tp: None if name in self.null else arr.ctypes.data_as(tp)
        return lib.sg_slam_optimize_pose_graph(
            None if "handle" in self.null else self.handle, None if "map" in self.null else C.byref(ms),
            a("fr", self.fr, IP), a("fx", self.fx, IP), a("noff", self.noff, IP), a("ab", self.ab, IP),
            a("meas", self.meas, DP), a("w", self.w, DP), a("eoff", self.eoff, IP), self.n,
            None if "o" in self.null else C.byref(self.o), a("status", self.status, IP), self.ls.ctypes.data_as(DP),
            self.sums)

    def untouched(self):
        return (_arrays(self.m) == self.before and bytes(self.buf.raw) == self.raw and (self.status == 77).all()
                and (self.ls == 7.5).all() and self.sums[0].num_iterations == 77)


def _mutations():
    def null(name):
        return lambda c: c.null.add(name)

    def setv(attr, idx, val):
        def f(c):
            getattr(c, attr)[idx] = val
        return f

    out = [("null " + n, null(n)) for n in ("handle", "map", "o", "fr", "fx", "noff", "ab", "meas", "w", "eoff", "status")]
    out += [("negative n", lambda c: setattr(c, "n", -1)),
            ("node_offset[0]", setv("noff", 0, 1)), ("edge_offset[0]", setv("eoff", 0, 1)),
            ("decreasing node offset", setv("noff", 1, -1)), ("decreasing edge offset", setv("eoff", 1, -1)),
            ("frame below range", setv("fr", 3, -1)), ("frame above range", setv("fr", 3, 8)),
            ("frame listed twice", setv("fr", 3, 2)),
            ("edge index below range", setv("ab", 5, -1)), ("edge index above range", setv("ab", 5, 8)),
            ("a == b", setv("ab", 5, 2)),
            ("q^ zero", lambda c: c.meas.__setitem__(slice(8, 12), 0.0)), ("q^ not unit", setv("meas", 11, 2.0)),
            ("q^ NaN", setv("meas", 9, np.nan)), ("u^ infinite", setv("meas", 13, np.inf)),
            ("rho^ NaN", setv("meas", 15, np.nan)),
            ("w_rot zero", setv("w", 3, 0.0)), ("w_t negative", setv("w", 4, -1.0)), ("w_s NaN", setv("w", 5, np.nan)),
            ("w_t infinite", setv("w", 4, np.inf)),
            ("range negative", lambda c: setattr(c.o, "range", -1.0)),
            ("range NaN", lambda c: setattr(c.o, "range", float("nan"))),
            ("range infinite", lambda c: setattr(c.o, "range", float("inf")))]
    return out


@pytest.mark.parametrize("what,mutate", _mutations(), ids=[w for w, _ in _mutations()])
def test_argument_errors_return_einval_with_nothing_written(what, mutate):
    lib = load_library()
    c = _Call()
    mutate(c)
    c.before = _arrays(c.m)
    assert c.run(lib) == -22, what
    assert c.untouched(), what
    assert lib.sg_last_error()


def test_size_caps_and_unreadable_maps_are_einval():
    lib = load_library()
    c = _Call()
    c.m.q = np.zeros(0)                 # poses that cannot be read
    c.before = _arrays(c.m)
    assert c.run(lib) == -22 and c.untouched()
    c = _Call()
    c.o.move_points = 1                 # observations out of range with move_points
    m = make_config("C1")
    m.obs_point[5] = m.num_points
    c.m, c.fr = m, np.arange(8, dtype=np.int32)
    c.before = _arrays(c.m)
    assert c.run(lib) == -22 and c.untouched()
    # more than 1024 nodes in a graph
    N = 1025
    c = _Call()
    c.m = pc.frames_map(np.tile([0.0, 0.0, 0.0, 1.0], (N, 1)), np.zeros((N, 3)))
    c.fr, c.fx = np.arange(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    c.noff = np.array([0, N], dtype=np.int32)
    c.before = _arrays(c.m)
    assert c.run(lib) == -22 and c.untouched()
    # more than 8192 edges in a graph
    c = _Call()
    E = 8193
    c.ab = np.tile(c.ab[:2], E)
    c.meas, c.w = np.tile(c.meas[:8], E), np.tile(c.w[:3], E)
    c.eoff = np.array([0, E], dtype=np.int32)
    assert c.run(lib) == -22 and c.untouched()


def test_no_graphs_returns_ok_before_anything_is_touched():
    lib = load_library()
    c = _Call()
    c.n = 0
    c.null |= {"fr", "fx", "noff", "ab", "meas", "w", "eoff", "status"}
    assert c.run(lib) == 0 and c.untouched()
    c.null.add("o")
    assert c.run(lib) == -22            # null options, even with n == 0


def test_statuses_decided_on_the_host_never_reach_the_device():
    lib = load_library()
    sc = pc.scene("two_comp")
    c = _Call("two_comp")
    # graph 0: two components, one unanchored; graph 1: all nodes fixed; graph 2: a free node no edge touches
    N = len(sc["q"])
    c.fr = np.arange(N, dtype=np.int32)
    c.noff = np.array([0, N, N, N], dtype=np.int32)
    c.eoff = np.array([0, len(sc["edges"]), len(sc["edges"]), len(sc["edges"])], dtype=np.int32)
    c.n = 3
    assert c.run(lib) == 0
    assert list(c.status[:3]) == [2, 1, 1] and c.status[3] == 77
    assert (c.ls[:N] == 0.0).all() and c.ls[N] == 7.5
    assert [c.sums[g].termination_type for g in range(3)] == [5, 5, 5] and c.sums[0].num_iterations == 0
    assert _arrays(c.m) == c.before and bytes(c.buf.raw) == c.raw     # frames untouched, handle never read
    c2 = _Call("ring8")
    c2.fx[:] = 1
    assert c2.run(lib) == 0 and c2.status[0] == 1 and _arrays(c2.m) == c2.before and bytes(c2.buf.raw) == c2.raw


# ------------------------------------------------------------------------------------------------ host-only helpers
def test_pose_edges_match_numpy_without_and_with_a_similarity():
    s = pc.host_slam()
    m = make_config("C1")
    q, t = m.q.reshape(-1, 4), m.t.reshape(-1, 3)
    pairs = np.array([[0, 1], [3, 7], [9, 2], [5, 4]], dtype=np.int32)
    before = _arrays(m)
    got = s.PoseEdges(m, pairs)
    want = pc.pose_edges_np(q, t, pairs)
    assert np.abs(got - want).max() <= 1e-12 * 1000.0 and (got[:, 3] >= 0).all() and (got[:, 7] == 0).all()
    sim = (1.3, pc.qunit([0.1, -0.2, 0.3, 0.9]), np.array([300.0, -200.0, 400.0]))
    got_s = s.PoseEdges(m, pairs, sim)
    want_s = pc.pose_edges_np(q, t, pairs, sim)
    assert np.abs(got_s - want_s).max() <= 1e-12 * 1000.0
    assert np.allclose(got_s[:, 7], -np.log(1.3), rtol=0, atol=1e-15)
    assert _arrays(m) == before                                        # the map is not written
    # moving the a frames with ApplySimilarity on a copy gives the same q^, and u^ s
    for a, b in pairs:
        mc = m.copy()
        s.ApplySimilarity(mc, sim[0], sim[1], sim[2], [a], [])
        one = s.PoseEdges(mc, [[a, b]])[0]
        ref = s.PoseEdges(m, [[a, b]], sim)[0]
        assert np.abs(one[:4] - ref[:4]).max() <= 1e-14
        assert np.abs(one[4:7] / sim[0] - ref[4:7]).max() <= 1e-12 * np.abs(one[4:7]).max()
    # the edge has zero residual at the states it describes
    x = np.zeros((m.num_frames, 8))
    x[:, :4], x[:, 4:7] = q, t
    for i, (a, b) in enumerate(pairs):
        r = pc.edge_residual(x[a], x[b], got[i], [pc.W_ROT, pc.W_T, pc.W_S], False)
        assert np.abs(r).max() <= 1e-9
    lib = load_library()
    ms = m.struct()
    out = np.full(8, 7.0)
    bad = np.array([0, 0], dtype=np.int32)
    for pr, simv in ((bad, None), (np.array([0, 10], dtype=np.int32), None), (np.array([-1, 1], dtype=np.int32), None),
                     (pairs[0], [0.0, 0, 0, 0, 1, 0, 0, 0]), (pairs[0], [1.0, 0, 0, 0, 2, 0, 0, 0]),
                     (pairs[0], [1.0, 0, 0, 0, 1, np.nan, 0, 0])):
        sv = None if simv is None else np.array(simv, dtype=np.float64).ctypes.data_as(DP)
        assert lib.sg_map_pose_edges(C.byref(ms), pr.ctypes.data_as(IP), 1, sv, out.ctypes.data_as(DP)) == -22
        assert (out == 7.0).all()
    assert lib.sg_map_pose_edges(None, pairs.ctypes.data_as(IP), 1, None, out.ctypes.data_as(DP)) == -22
    assert lib.sg_map_pose_edges(C.byref(ms), None, 0, None, None) == 0


def _covisible_np(m, frames, min_shared):
    usable = (m.point_flags & 0b10111) == 0
    seen = [set(int(p) for f, p, d in zip(m.obs_frame, m.obs_point, m.obs_disabled) if f == fr and not d and usable[p])
            for fr in frames]
    return [(i, j) for i in range(len(frames)) for j in range(i + 1, len(frames))
            if len(seen[i] & seen[j]) >= min_shared]


def test_covisible_pairs_match_a_set_count_and_fill_in_two_calls():
    s = pc.host_slam()
    lib = load_library()
    m = make_config("C1")
    m.obs_disabled[::7] = 1
    m.point_flags[::5] = 1 << 1          # NO_BASELINE: not usable
    m.point_flags[1::5] = 1 << 3         # MISMATCHED: usable
    frames = np.array([9, 0, 4, 3, 7, 1, 8], dtype=np.int32)
    for min_shared in (1, 20, 60, 10 ** 6):
        want = _covisible_np(m, frames, min_shared)
        got = s.CovisiblePairs(m, frames, min_shared)
        assert [tuple(p) for p in got] == want, min_shared
    want = _covisible_np(m, frames, 20)
    assert len(want) > 3
    ms = m.struct()
    cnt = C.c_int32(-1)
    out = np.full(2 * 3 + 2, 77, dtype=np.int32)
    assert lib.sg_map_covisible_pairs(C.byref(ms), frames.ctypes.data_as(IP), len(frames), 20, out.ctypes.data_as(IP), 3,
                                      C.byref(cnt)) == 0
    assert cnt.value == len(want) and [tuple(p) for p in out[:6].reshape(3, 2)] == want[:3] and (out[6:] == 77).all()
    for fr, nf, ms_, cap in ((frames, len(frames), 0, 3), (frames, -1, 20, 3), (frames, len(frames), 20, -1),
                             (np.array([0, 0], dtype=np.int32), 2, 20, 3), (np.array([0, 10], dtype=np.int32), 2, 20, 3)):
        assert lib.sg_map_covisible_pairs(C.byref(ms), fr.ctypes.data_as(IP), nf, ms_, out.ctypes.data_as(IP), cap,
                                          C.byref(cnt)) == -22
    assert lib.sg_map_covisible_pairs(C.byref(ms), frames.ctypes.data_as(IP), len(frames), 20, None, 3, C.byref(cnt)) == -22


# ------------------------------------------------------------------------------------------------ the CPU executor
@pytest.mark.parametrize("name", pc.SCENES)
def test_cpu_executor_solves_every_scene_as_the_reference_does(name):
    s = pc.host_slam()
    sc, ref = pc.scene(name), pc.reference(name)
    m = pc.frames_map(sc["q"], sc["t"])
    out = s.OptimizePoseGraph(m, [pc.graph_of(sc)], range_=sc["range"], fix_scale=sc["fix_scale"], cpu=True,
                              options=pc.solver_options(name))[0]
    assert out["status"] == "OK" and out["termination"] == ref["termination"]
    for key in ("num_iterations", "num_successful_steps", "num_unsuccessful_steps", "num_invalid_steps"):
        assert out[key] == ref[key], key
    d = pc.compare(pc.states(m, np.arange(len(sc["q"])), out["log_scale"]), ref["x"])
    d["cost"] = abs(out["final_cost"] - ref["final_cost"])
    print(name, d)
    for key, val in d.items():
        assert val <= pc.bound(name, key), (key, val, pc.bound(name, key))
    fixed = np.flatnonzero(sc["fixed"])
    assert (m.q.reshape(-1, 4)[fixed] == sc["q"][fixed]).all() and (m.t.reshape(-1, 3)[fixed] == sc["t"][fixed]).all()
    if name == "complete48":
        # the scene is there for the strided loops' second trip: column j of a complete graph's 47 has 46 - j rows
        rows = [r for _, r in pc.column_rows(sc)]
        assert rows == list(range(46, -1, -1)) and sum(7 * r > 256 for r in rows) == 10


@pytest.mark.parametrize("name", pc.PATH_SCENES)
def test_cpu_executor_takes_the_paths_that_do_not_end_converged(name):
    s = pc.host_slam()
    sc = pc.scene(name)
    m = pc.frames_map(sc["q"], sc["t"])
    before = m.copy()
    out = s.OptimizePoseGraph(m, [pc.graph_of(sc)], range_=sc["range"], fix_scale=sc["fix_scale"], cpu=True,
                              options=pc.solver_options(name))[0]
    pc.check_path_result(name, out, m, before)


def test_cpu_executor_solves_cap1024_behind_another_graph():
    """A graph at the node cap behind complete48 in one call (large node0, col0 and block offsets), against the
    committed reference result: the plan and the index arithmetic the kernel shares, without a device."""
    s = pc.host_slam()
    scs = [pc.scene("complete48"), pc.scene("cap1024")]
    m = pc.frames_map(np.vstack([sc["q"] for sc in scs]), np.vstack([sc["t"] for sc in scs]))
    graphs = [pc.graph_of(scs[0], np.arange(48)), pc.graph_of(scs[1], 48 + np.arange(1024))]
    out = s.OptimizePoseGraph(m, graphs, cpu=True)
    assert out[0]["status"] == "OK" and out[0]["num_iterations"] == pc.reference("complete48")["num_iterations"]
    pc.check_cap1024(pc.states(m, 48 + np.arange(1024), out[1]["log_scale"]), out[1])


def _drifted_c1():
    """C1 at its true poses and points, with a smooth drift planted on the later frames, and the graph that undoes it:
    odometry edges of the true trajectory, frames 0 and 1 fixed."""
    m = make_config("C1", perturb=False)
    F = m.num_frames
    q, t = m.q.reshape(-1, 4).copy(), m.t.reshape(-1, 3).copy()
    pairs = np.array([(i, i + 1) for i in range(F - 1)] + [(i, i + 2) for i in range(F - 2)], dtype=np.int32)
    meas = pc.pose_edges_np(q, t, pairs)
    meas[:, 7] = [0.01 * (b - a) for a, b in pairs]          # the map's scale grows along the run
    rng = np.random.default_rng(3)
    fixed = np.zeros(F, dtype=np.int32)
    fixed[:2] = 1
    m.q[:], m.t[:] = (v.reshape(-1) for v in pc._perturbed(q, t, fixed, rng, 1.0, 15.0))
    graph = {"frames": np.arange(F), "fixed": fixed, "edges": pairs, "meas": meas,
             "weights": np.tile([pc.W_ROT, pc.W_T, pc.W_S], (len(pairs), 1))}
    return m, graph


def test_move_points_follows_the_formula_and_keeps_the_anchor_frames_pixels():
    s = pc.host_slam()
    m, graph = _drifted_c1()
    m.obs_disabled[::9] = 1
    old = m.copy()
    flags, dis = m.point_flags.copy(), m.obs_disabled.copy()
    out = s.OptimizePoseGraph(m, [graph], move_points=True, cpu=True)[0]
    assert out["status"] == "OK"
    assert (m.point_flags == flags).all() and (m.obs_disabled == dis).all()
    ls = out["log_scale"]
    assert ls[0] == ls[1] == 0.0 and np.ptp(ls) > 0.05
    Xo, Xn = old.X.reshape(-1, 4), m.X.reshape(-1, 4)
    qo, to, qn, tn = old.q.reshape(-1, 4), old.t.reshape(-1, 3), m.q.reshape(-1, 4), m.t.reshape(-1, 3)
    anchor = np.full(m.num_points, -1)
    for f, p, d in zip(m.obs_frame, m.obs_point, m.obs_disabled):
        if not d and anchor[p] < 0:
            anchor[p] = f
    moved = 0
    for p in range(m.num_points):
        f = anchor[p]
        if f < 0 or graph["fixed"][f]:
            assert (Xn[p] == Xo[p]).all()
            continue
        moved += 1
        W = Xo[p, 3]
        want = np.exp(ls[f]) * quat_to_matrix(qn[f]).T @ quat_to_matrix(qo[f]) @ (Xo[p, :3] - W * to[f]) + W * tn[f]
        assert Xn[p, 3] == W and np.abs(Xn[p, :3] - want).max() <= 1e-12 * np.abs(want).max()
        # the anchor frame's pixel of the point does not move
        k = m.k[7 * m.frame_camera[f]:7 * m.frame_camera[f] + 7]
        uo, ok0 = project_np(quat_to_matrix(qo[f])[None], to[f][None], k, (Xo[p, :3] / W)[None])
        un, ok1 = project_np(quat_to_matrix(qn[f])[None], tn[f][None], k, (Xn[p, :3] / W)[None])
        assert ok0[0] and ok1[0] and np.abs(uo - un).max() <= 1e-9
    assert moved > 300
    # without move_points no point moves
    m2 = old.copy()
    s.OptimizePoseGraph(m2, [graph], move_points=False, cpu=True)
    assert (m2.X == old.X).all() and (m2.q == m.q).all() and (m2.t == m.t).all()
