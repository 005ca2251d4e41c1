"""Times sg_slam_match_by_projection (Slam.MatchByProjection) on an MI355X and writes profiles/match_bench.json.

Rows: frame 8 of C1 with its keypoints against the 484 points of C1; one C2 frame with 2000 keypoints against all
19,449 points of C2; all 50 C2 frames, 2000 keypoints each, in one call.  Keypoints as in tests/match_cases.py: the
frame's observation pixels with the landmark's descriptor after Binomial(256, 0.03) bit flips, and distractors; every
second observation of the map is disabled, and skip_observed is on.  Per row: the median wall time of the call over
--repeats calls after --warmup (the Python wrapper included), and the HIP-event time of its three launches.  For
scale, in the same session: the all-pairs sg_hamming_match on the same 2000 x 19,449 descriptors, its wall time and
the HIP-event time of its two launches.

    python tools/match_bench.py [--repeats 20] [--warmup 3]
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

import match_cases as mc  # noqa: E402
from slamgpu import ba  # noqa: E402
from slamgpu.matcher import HammingMatcher  # noqa: E402
from slamgpu.scene import make_config  # noqa: E402


def _scene(name):
    m = make_config(name, noise=0.0, outlier_frac=0.0, perturb=False)
    m.obs_disabled[1::2] = 1
    return m, mc._random_desc(np.random.default_rng(8), m.num_points)


def _keypoints(m, desc, f, limit):
    xy, kd = mc.frame_keypoints(m, desc, f, 2000 + f)
    return xy[:limit], kd[:limit]


def _time(call, s, repeats, warmup):
    on, ms = s.lib.sg_slam_debug_match_timing, s.lib.sg_slam_debug_match_kernel_ms
    on.argtypes = [C.c_void_p, C.c_int32]
    ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    wall, kern = [], []
    for i in range(warmup + repeats):
        if i == warmup:
            on(s.h, 1)
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            v = C.c_double()
            ms(s.h, C.byref(v))
            wall.append(dt)
            kern.append(v.value)
    return {"wall_ms_median": statistics.median(wall), "kernel_ms_median": statistics.median(kern),
            "wall_ms_min": min(wall), "wall_ms_max": max(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.json"))
    a = ap.parse_args()
    rows = []
    c1, c2 = _scene("C1"), _scene("C2")
    cases = (("C1, frame 8", c1, [8], 10 ** 6), ("C2, frame 25, 2000 keypoints", c2, [25], 2000),
             ("C2, all 50 frames, 2000 keypoints each", c2, list(range(50)), 2000))
    for label, (m, desc), frames, limit in cases:
        kps = [_keypoints(m, desc, f, limit) for f in frames]
        points = np.arange(m.num_points, dtype=np.int32)
        s = ba.Slam()
        t = _time(lambda: s.MatchByProjection(m, frames, kps, points, desc, radius_px=mc.RADIUS), s, a.repeats, a.warmup)
        res = s.projection_match_results()
        nc = np.concatenate([r["num_candidates"] for r in res])
        row = dict(case=label, call="MatchByProjection", frames=len(frames), keypoints=int(sum(len(k[0]) for k in kps)),
                   points=int(m.num_points), projected=int(sum(r["num_projected"] for r in res)),
                   mean_window=float(nc.mean()), matched=int(sum(r["num_matched"] for r in res)), **t)
        print(json.dumps(row))
        rows.append(row)
    # for scale: all-pairs Hamming on the descriptors of the one-frame C2 row
    m, desc = c2
    kd = _keypoints(m, desc, 25, 2000)[1]
    hm = HammingMatcher(device=0)
    wall, kern = [], []
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        hm.match(kd, desc)
        dt = (time.perf_counter() - t0) * 1e3
        hm.load(kd, desc)
        hm.run(1)
        ms = hm.results()[3]
        if i >= a.warmup:
            wall.append(dt)
            kern.append(ms)
    hm.close()
    row = dict(case="C2 descriptors, 2000 x %d" % len(desc), call="sg_hamming_match", frames=1, keypoints=len(kd),
               points=len(desc), wall_ms_median=statistics.median(wall), kernel_ms_median=statistics.median(kern),
               wall_ms_min=min(wall), wall_ms_max=max(wall))
    print(json.dumps(row))
    rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/match_bench.py", "repeats": a.repeats, "warmup": a.warmup, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
