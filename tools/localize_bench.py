#!/usr/bin/env python3
"""Times localization from scratch (Slam.LocalizeFrames: k_pose_ransac, k_pose_select and, with the polish, k_pose_lm
and k_pose_select again) on three workloads: one frame of config 1, the newest 5 frames of config 2 and all 50 frames
of config 2, at max_hypotheses 1024 and 8192, without and with the polish.  30 % of each listed frame's records are
replaced by random pixels and the entry poses by garbage, so the work is what a relocalization does.  Per shape: the
host wall time of the call (it ends in the download's device synchronisation) and the HIP-event time from before the
first launch to after the last, each the median of --repeats calls after --warmup calls, every call on a fresh copy
of the map.  Beside them, for scale, SolveFramePoses on the same frames from the true poses 60 mm off in x (a
start inside its basin), timed by the same protocol in the same session.  Prints one JSON line.

    python tools/localize_bench.py [--repeats 30] [--warmup 5] [--out FILE]
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
from slamgpu.capi import check   # noqa: E402
from slamgpu.scene import HEIGHT, WIDTH, make_config   # noqa: E402

RANGE = 2.0
TAU = 4.0
OUTLIER_SHARE = 0.3


def relocalization_map(name, frames):
    """Config `name` with the true points, 30 % random pixels in each listed frame and garbage entry poses there."""
    m = make_config(name, perturb=False, outlier_frac=0.0)
    rng = np.random.default_rng(7)
    pts = m.obs_pt.reshape(-1, 2)
    for f in frames:
        sel = np.flatnonzero(m.obs_frame == f)
        out = rng.choice(sel, size=int(round(OUTLIER_SHARE * len(sel))), replace=False)
        pts[out] = rng.uniform((0.0, 0.0), (WIDTH, HEIGHT), size=(len(out), 2))
    local = m.copy()           # the local solver's start: the truth, 60 mm off in x
    local.t[0::3] += 60.0
    for f in frames:
        m.q[4 * f:4 * f + 4] = (0.5, -0.5, 0.5, 0.5)
        m.t[3 * f:3 * f + 3] = (1e5, -2e5, 3e5)
    return m, local


def time_calls(slam, call, m, repeats, warmup, kernel):
    """Median, min, max ms over `repeats` calls: the call's wall time, or (kernel) the launches' HIP-event time."""
    lib = slam.lib
    check(lib.sg_slam_debug_pose_timing(slam.h, int(kernel)), "sg_slam_debug_pose_timing")
    out = []
    for i in range(warmup + repeats):
        mc = m.copy()
        t0 = time.perf_counter()
        solved = call(mc)
        wall = (time.perf_counter() - t0) * 1e3
        assert all(solved), solved
        if kernel:
            ms = C.c_double()
            check(lib.sg_slam_debug_pose_kernel_ms(slam.h, C.byref(ms)), "sg_slam_debug_pose_kernel_ms")
            wall = ms.value
        if i >= warmup:
            out.append(wall)
    check(lib.sg_slam_debug_pose_timing(slam.h, 0), "sg_slam_debug_pose_timing")
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    slam = ba.Slam()
    lib = slam.lib
    lib.sg_slam_debug_pose_timing.argtypes = [C.c_void_p, C.c_int32]
    lib.sg_slam_debug_pose_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    res = {"tool": "localize_bench", "threshold_px": TAU, "range": RANGE, "outlier_share": OUTLIER_SHARE,
           "repeats": a.repeats, "warmup": a.warmup, "workloads": {}}
    for label, name, pick in (("C1 newest frame", "C1", lambda F: [F - 1]),
                              ("C2 newest 5 frames", "C2", lambda F: list(range(F - 5, F))),
                              ("C2 all 50 frames", "C2", lambda F: list(range(F)))):
        F = make_config(name).num_frames
        frames = pick(F)
        m, local = relocalization_map(name, frames)
        w = {"config": name, "frames": len(frames),
             "records": int(sum(np.count_nonzero(m.obs_frame == f) for f in frames)), "localize": {}}
        for H in (1024, 8192):
            for refine in (False, True):
                def call(mc, H=H, refine=refine):
                    return slam.LocalizeFrames(mc, frames, threshold_px=TAU, max_hypotheses=H, refine=refine,
                                               range_=RANGE)
                mc = m.copy()
                call(mc)
                r = slam.localization_results()
                off = max(np.abs(mc.t[3 * f:3 * f + 3] - m.t_true[3 * f:3 * f + 3]).max() for f in frames)
                w["localize"]["H%d%s" % (H, "_refine" if refine else "")] = {
                    "max_hypotheses": H, "refine": int(refine),
                    "localized": int(sum(x["status"] == "OK" for x in r)), "refined": int(sum(x["refined"] for x in r)),
                    "inliers": int(sum(x["num_inliers"] for x in r)), "worst_translation_error": float(off),
                    "wall_ms": time_calls(slam, call, m, a.repeats, a.warmup, kernel=False),
                    "kernel_ms": time_calls(slam, call, m, a.repeats, a.warmup, kernel=True)}

        def local_call(mc):
            return slam.SolveFramePoses(mc, frames, RANGE)
        w["solve_frame_poses_same_session"] = {
            "wall_ms": time_calls(slam, local_call, local, a.repeats, a.warmup, kernel=False),
            "kernel_ms": time_calls(slam, local_call, local, a.repeats, a.warmup, kernel=True)}
        res["workloads"][label] = w
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
