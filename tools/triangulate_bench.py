#!/usr/bin/env python3
"""Times linear multi-view triangulation (Slam.TriangulatePoints, k_point_triangulate) on the four lists of
tools/points_bench.py: 120 points of the newest frame of C2 (a keyframe's seeds), the points seen by the newest 5
frames of C2, every point of C2 and every point of C5, gates off, with refine = 0 (one launch) and refine = 1
(k_point_lm from the triangulated locations on the same stream).  The location at entry is not read, so the calls
need no fresh start.  Per list and mode: the host wall time of the C call (planner, upload, launches, download; it
ends in the download's device synchronisation) and the HIP-event time from before the first launch to after the
last, each the median of --repeats calls after --warmup calls.  Run tools/points_bench.py in the same session for
k_point_lm's own times on the same lists.  Prints one JSON line.

    python tools/triangulate_bench.py [--repeats 20] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "slam-robot_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np   # noqa: E402

from slamgpu import ba   # noqa: E402
from slamgpu.capi import SgTriangulateOptions, check   # noqa: E402
from slamgpu.scene import make_config   # noqa: E402

RANGE = 2.0


def time_calls(slam, m, points, refine, repeats, warmup, kernel):
    """Median ms over `repeats` calls of sg_slam_triangulate_points itself (what a C++ caller pays; the Python
    mirror's per-point dicts are left out): the call's wall time, or (kernel) the launches' HIP-event time."""
    lib = slam.lib
    check(lib.sg_slam_debug_points_timing(slam.h, int(kernel)), "sg_slam_debug_points_timing")
    X0 = m.X.copy()
    ms_, ip = m.struct(), C.POINTER(C.c_int32)
    opt = SgTriangulateOptions(min_parallax=0.0, max_error_px=0.0, refine=int(refine), range=RANGE)
    solved = np.zeros(len(points), dtype=np.int32)
    out = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        rc = lib.sg_slam_triangulate_points(slam.h, C.byref(ms_), points.ctypes.data_as(ip), len(points),
                                            C.byref(opt), solved.ctypes.data_as(ip), None, None)
        wall = (time.perf_counter() - t0) * 1e3
        check(rc, "sg_slam_triangulate_points")
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    slam = ba.Slam()
    lib = slam.lib
    lib.sg_slam_debug_points_timing.argtypes = [C.c_void_p, C.c_int32]
    lib.sg_slam_debug_points_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    res = {"tool": "triangulate_bench", "range": RANGE, "repeats": a.repeats, "warmup": a.warmup, "shapes": {}}
    c2 = make_config("C2")
    F = c2.num_frames
    newest = np.unique(c2.obs_point[c2.obs_frame == F - 1])
    newest5 = np.unique(c2.obs_point[c2.obs_frame >= F - 5])
    shapes = [("C2_seeds_120", c2, newest[:120]), ("C2_newest_5_frames", c2, newest5),
              ("C2_all", c2, np.arange(c2.num_points))]
    c5 = make_config("C5")
    shapes.append(("C5_all", c5, np.arange(c5.num_points)))
    for name, m, points in shapes:
        points = np.ascontiguousarray(points, dtype=np.int32)
        X0 = m.X.copy()
        solved = slam.TriangulatePoints(m, points, refine=True, range_=RANGE)
        st = [r["status"] for r in slam.triangulation_results()]
        sums = [s for s in slam.point_summaries() if s["termination"] != "DID_NOT_RUN"]
        m.X[:] = X0
        listed = np.zeros(m.num_points, dtype=bool)
        listed[points] = True
        row = {
            "frames": int(m.num_frames), "points": int(len(points)), "solved": int(sum(solved)),
            "observations": int(np.count_nonzero(listed[m.obs_point] & (m.obs_disabled == 0))),
            "statuses": {k: st.count(k) for k in sorted(set(st))},
            "lm_iterations_max": max(s["num_lm_iterations"] for s in sums),
            "lm_iterations_mean": sum(s["num_lm_iterations"] for s in sums) / len(sums),
        }
        for refine in (0, 1):
            wall = time_calls(slam, m, points, refine, a.repeats, a.warmup, kernel=False)
            kern = time_calls(slam, m, points, refine, a.repeats, a.warmup, kernel=True)
            row["refine_%d" % refine] = {
                "wall_ms_median": wall[0], "wall_ms_min": wall[1], "wall_ms_max": wall[2],
                "kernel_ms_median": kern[0], "kernel_ms_min": kern[1], "kernel_ms_max": kern[2]}
        res["shapes"][name] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
