#!/usr/bin/env python3
"""Times pose-only bundle adjustment (Slam.SolveFramePoses, k_pose_lm) on the C1 and C2 maps: one frame per call
and every frame in one call.  Per shape: the host wall time of the call (it ends in the download's device
synchronisation) and the HIP-event time of the k_pose_lm launch, each the median of --repeats calls after
--warmup calls, every call on a fresh copy of the map (a solved pose would converge at once); beside them the CPU
oracle's time for the same per-frame problems.  Prints one JSON line.

    python tools/pose_bench.py [--repeats 30] [--warmup 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-robot_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402

import oracle   # noqa: E402
from slamgpu import ba   # noqa: E402
from slamgpu.capi import ProblemArrays, check   # noqa: E402
from slamgpu.scene import make_config   # noqa: E402

RANGE = 2.0
UNUSABLE = (1 << 0) | (1 << 1) | (1 << 2) | (1 << 4)


def pose_problem(m, f):
    """The per-frame Ceres problem of sg_slam_solve_frame_poses (frame f free, every point constant)."""
    sel = np.flatnonzero((m.obs_frame == f) & (m.obs_disabled == 0) & ((m.point_flags[m.obs_point] & UNUSABLE) == 0))
    pts, inv = np.unique(m.obs_point[sel], return_inverse=True)
    return ProblemArrays(
        k=m.k.copy(), q=m.q[4 * f:4 * f + 4].copy(), t=m.t[3 * f:3 * f + 3].copy(),
        frame_camera=m.frame_camera[[f]], frame_rot_free=[1], frame_trans_free=[1], X=m.X.reshape(-1, 4)[pts].copy(),
        point_free=np.zeros(len(pts), dtype=np.uint8), obs_pt=m.obs_pt.reshape(-1, 2)[sel].copy(),
        obs_frame=np.zeros(len(sel), dtype=np.int32), obs_point=inv, dist_frame=[], dist_prev=[], range_=RANGE)


def time_calls(slam, m, frames, repeats, warmup, kernel):
    """Median ms over `repeats` calls: the call's wall time, or (kernel) the launch's HIP-event time."""
    lib = slam.lib
    check(lib.sg_slam_debug_pose_timing(slam.h, int(kernel)), "sg_slam_debug_pose_timing")
    out = []
    for i in range(warmup + repeats):
        mc = m.copy()
        t0 = time.perf_counter()
        solved = slam.SolveFramePoses(mc, frames, RANGE)
        wall = (time.perf_counter() - t0) * 1e3
        assert any(solved), solved
        if kernel:
            ms = C.c_double()
            check(lib.sg_slam_debug_pose_kernel_ms(slam.h, C.byref(ms)), "sg_slam_debug_pose_kernel_ms")
            wall = ms.value
        if i >= warmup:
            out.append(wall)
    check(lib.sg_slam_debug_pose_timing(slam.h, 0), "sg_slam_debug_pose_timing")
    return statistics.median(out), min(out), max(out)


def oracle_ms(m, frames, repeats=3):
    best = []
    for _ in range(repeats):
        pas = [pose_problem(m, f) for f in frames]
        t0 = time.perf_counter()
        for pa in pas:
            oracle.solve(pa)
        best.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(best)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    oracle.build()
    slam = ba.Slam()
    lib = slam.lib
    lib.sg_slam_debug_pose_timing.argtypes = [C.c_void_p, C.c_int32]
    lib.sg_slam_debug_pose_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    res = {"tool": "pose_bench", "range": RANGE, "repeats": a.repeats, "warmup": a.warmup, "configs": {}}
    for name in ("C1", "C2"):
        m = make_config(name)
        F = m.num_frames
        cfg = {"frames": F, "observations": int(m.num_obs)}
        for shape, frames in (("single", [F - 1]), ("all", list(range(F)))):
            mc = m.copy()
            solved = slam.SolveFramePoses(mc, frames, RANGE)
            sums = slam.frame_pose_summaries()
            wall = time_calls(slam, m, frames, a.repeats, a.warmup, kernel=False)
            kern = time_calls(slam, m, frames, a.repeats, a.warmup, kernel=True)
            cfg[shape] = {
                "frames": len(frames), "solved": int(sum(solved)),
                "observations": int(sum(np.count_nonzero(m.obs_frame == f) for f in frames)),
                "lm_iterations_max": max(s["num_lm_iterations"] for s in sums),
                "lm_iterations_sum": sum(s["num_lm_iterations"] for s in sums),
                "wall_ms_median": wall[0], "wall_ms_min": wall[1], "wall_ms_max": wall[2],
                "kernel_ms_median": kern[0], "kernel_ms_min": kern[1], "kernel_ms_max": kern[2],
                "oracle_cpu_ms": oracle_ms(m, frames),
            }
        res["configs"][name] = cfg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
