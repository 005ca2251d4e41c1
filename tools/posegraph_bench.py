"""Times sg_slam_optimize_pose_graph (Slam.OptimizePoseGraph) on an MI355X and writes profiles/posegraph_bench.json.

Rows: a 50-node ring with covisibility edges to the next 3 frames; a 200-node one (config 5's frame count); 16 graphs
of 50 nodes in one call.  Measurements are exact, node 0 of each graph is fixed and the others start 1 degree and 10 map
units off.  Per row: the median wall time of the call over --repeats calls after --warmup, the HIP-event time of its
one launch, and beside it the wall time of the planner's CPU executor doing the same LM on the host in the same session
(sg_posegraph_debug_cpu_solve: the same plan and arithmetic, one thread; the only baseline there is), the planning
included in both.

    python tools/posegraph_bench.py [--repeats 10] [--warmup 2]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-robot_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import posegraph_cases as pc  # noqa: E402
from slamgpu import ba  # noqa: E402


def _ring(N, seed):
    ed = [(i, (i + k) % N) for i in range(N) for k in (1, 2, 3)]
    return pc._exact("ring%d" % N, N, ed, [0], seed, radius=20.0 * N, rot_deg=1.0, trans=10.0)


def _call(scenes):
    q = np.vstack([s["q"] for s in scenes])
    t = np.vstack([s["t"] for s in scenes])
    off = np.cumsum([0] + [len(s["q"]) for s in scenes])
    return pc.frames_map(q, t), [pc.graph_of(s, np.arange(off[i], off[i + 1])) for i, s in enumerate(scenes)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_bench.json"))
    a = ap.parse_args()
    s = ba.Slam()
    on, ms = s.lib.sg_slam_debug_posegraph_timing, s.lib.sg_slam_debug_posegraph_kernel_ms
    on.argtypes = [C.c_void_p, C.c_int32]
    ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    rows = []
    cases = (("one ring of 50 nodes", [_ring(50, 50)]), ("one ring of 200 nodes", [_ring(200, 200)]),
             ("16 rings of 50 nodes in one call", [_ring(50, 100 + i) for i in range(16)]))
    for label, scenes in cases:
        m0, graphs = _call(scenes)
        wall, kern, cpu = [], [], []
        out = out_cpu = None
        for i in range(a.warmup + a.repeats):
            on(s.h, 1)
            m = m0.copy()
            t0 = time.perf_counter()
            out = s.OptimizePoseGraph(m, graphs)
            dt = (time.perf_counter() - t0) * 1e3
            v = C.c_double()
            ms(s.h, C.byref(v))
            mc = m0.copy()
            t0 = time.perf_counter()
            out_cpu = s.OptimizePoseGraph(mc, graphs, cpu=True)
            dc = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                wall.append(dt)
                kern.append(v.value)
                cpu.append(dc)
        row = dict(case=label, graphs=len(graphs), nodes=int(sum(len(g["frames"]) for g in graphs)),
                   edges=int(sum(len(g["edges"]) for g in graphs)), solved=int(sum(o["status"] == "OK" for o in out)),
                   iterations=[o["num_iterations"] for o in out][:4], lm_iterations=out[0]["num_lm_iterations"],
                   same_counts_as_cpu=bool(all(o["num_iterations"] == c["num_iterations"] for o, c in zip(out, out_cpu))),
                   worst_pose_gap_to_cpu=float(np.abs(m.t - mc.t).max()),
                   wall_ms_median=statistics.median(wall), kernel_ms_median=statistics.median(kern),
                   wall_ms_min=min(wall), wall_ms_max=max(wall), cpu_executor_wall_ms_median=statistics.median(cpu))
        print(json.dumps(row))
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/posegraph_bench.py", "repeats": a.repeats, "warmup": a.warmup, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
