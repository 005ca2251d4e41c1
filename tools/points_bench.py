#!/usr/bin/env python3
"""Times structure-only bundle adjustment (Slam.SolvePoints, k_point_lm) on four shapes: 120 points of the newest
frame of C2 (a keyframe's seeds), the points seen by the newest 5 frames of C2, every point of C2 and every point
of C5.  Every point starts with its depth off by -40 .. +60 % along the ray from its first observing frame and a
small tilt.  Per shape: the host wall time of the C call (planner, upload, launch, download; it ends in the
download's device synchronisation) and the HIP-event time of the k_point_lm launch, each the median of
--repeats calls after --warmup calls, every call on a fresh copy of the points (a solved point would converge at
once); for the 120-point shape also the CPU oracle's time for the same per-point problems.  Prints one JSON line.

    python tools/points_bench.py [--repeats 20] [--warmup 3] [--out FILE]
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


def start(m, seed=1):
    """Every point's depth off by -40 .. +60 % along the ray from its first observing frame, and a small tilt."""
    rng = np.random.default_rng(seed)
    P = m.num_points
    X = m.X.reshape(-1, 4)
    pts, first = np.unique(m.obs_point, return_index=True)
    c = np.zeros((P, 3))
    c[pts] = m.t.reshape(-1, 3)[m.obs_frame[first]]
    Xe = c + (X[:, :3] / X[:, 3:] - c) / rng.uniform(0.6, 1.6, (P, 1))
    Xh = np.concatenate([Xe, np.ones((P, 1))], 1)
    X[:] = Xh / np.linalg.norm(Xh, axis=1, keepdims=True)
    X[:, :3] += rng.normal(0, 2e-3, (P, 3))
    return m


def point_problem(m, p):
    """The per-point Ceres problem of sg_slam_solve_points (point p free, every frame constant)."""
    sel = np.flatnonzero((m.obs_point == p) & (m.obs_disabled == 0))
    fr, inv = np.unique(m.obs_frame[sel], return_inverse=True)
    z = np.zeros(len(fr), dtype=np.uint8)
    return ProblemArrays(
        k=m.k.copy(), q=m.q.reshape(-1, 4)[fr].copy(), t=m.t.reshape(-1, 3)[fr].copy(), frame_camera=m.frame_camera[fr],
        frame_rot_free=z, frame_trans_free=z, X=m.X[4 * p:4 * p + 4].copy(), point_free=[1],
        obs_pt=m.obs_pt.reshape(-1, 2)[sel].copy(), obs_frame=inv, obs_point=np.zeros(len(sel), dtype=np.int32),
        dist_frame=[], dist_prev=[], range_=RANGE)


def time_calls(slam, m, points, repeats, warmup, kernel):
    """Median ms over `repeats` calls of sg_slam_solve_points itself (what a C++ caller pays; the Python mirror's
    per-point summary dicts are left out): the call's wall time, or (kernel) the launch's HIP-event time."""
    lib = slam.lib
    check(lib.sg_slam_debug_points_timing(slam.h, int(kernel)), "sg_slam_debug_points_timing")
    X0 = m.X.copy()
    ms_, ip = m.struct(), C.POINTER(C.c_int32)
    solved = np.zeros(len(points), dtype=np.int32)
    out = []
    for i in range(warmup + repeats):
        m.X[:] = X0
        t0 = time.perf_counter()
        rc = lib.sg_slam_solve_points(slam.h, C.byref(ms_), points.ctypes.data_as(ip), len(points), RANGE,
                                      solved.ctypes.data_as(ip), None)
        wall = (time.perf_counter() - t0) * 1e3
        check(rc, "sg_slam_solve_points")
        assert solved.any()
        if kernel:
            ms = C.c_double()
            check(lib.sg_slam_debug_points_kernel_ms(slam.h, C.byref(ms)), "sg_slam_debug_points_kernel_ms")
            wall = ms.value
        if i >= warmup:
            out.append(wall)
    m.X[:] = X0
    check(lib.sg_slam_debug_points_timing(slam.h, 0), "sg_slam_debug_points_timing")
    return statistics.median(out), min(out), max(out)


def oracle_ms(m, points):
    pas = [point_problem(m, p) for p in points]
    t0 = time.perf_counter()
    for pa in pas:
        oracle.solve(pa)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    oracle.build()
    slam = ba.Slam()
    lib = slam.lib
    lib.sg_slam_debug_points_timing.argtypes = [C.c_void_p, C.c_int32]
    lib.sg_slam_debug_points_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    res = {"tool": "points_bench", "range": RANGE, "repeats": a.repeats, "warmup": a.warmup, "shapes": {}}
    c2 = start(make_config("C2"))
    F = c2.num_frames
    newest = np.unique(c2.obs_point[c2.obs_frame == F - 1])
    newest5 = np.unique(c2.obs_point[c2.obs_frame >= F - 5])
    shapes = [("C2_seeds_120", c2, newest[:120]), ("C2_newest_5_frames", c2, newest5),
              ("C2_all", c2, np.arange(c2.num_points))]
    c5 = start(make_config("C5"))
    shapes.append(("C5_all", c5, np.arange(c5.num_points)))
    for name, m, points in shapes:
        points = np.ascontiguousarray(points, dtype=np.int32)
        X0 = m.X.copy()
        solved = slam.SolvePoints(m, points, RANGE)
        sums = slam.point_summaries()
        m.X[:] = X0
        listed = np.zeros(m.num_points, dtype=bool)
        listed[points] = True
        wall = time_calls(slam, m, points, a.repeats, a.warmup, kernel=False)
        kern = time_calls(slam, m, points, a.repeats, a.warmup, kernel=True)
        res["shapes"][name] = {
            "frames": int(m.num_frames), "points": int(len(points)), "solved": int(sum(solved)),
            "observations": int(np.count_nonzero(listed[m.obs_point] & (m.obs_disabled == 0))),
            "lm_iterations_max": max(s["num_lm_iterations"] for s in sums),
            "lm_iterations_mean": sum(s["num_lm_iterations"] for s in sums) / len(sums),
            "wall_ms_median": wall[0], "wall_ms_min": wall[1], "wall_ms_max": wall[2],
            "kernel_ms_median": kern[0], "kernel_ms_min": kern[1], "kernel_ms_max": kern[2],
        }
        if len(points) <= 120:
            res["shapes"][name]["oracle_cpu_ms"] = oracle_ms(m, points)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
