"""Times sg_slam_align_points (Slam.AlignPoints) on an MI355X and writes profiles/align_bench.json.

Rows: one group of 200 C1 landmarks; 49 groups built from C2 (group i: the landmarks frames i and i + 1 both see); one
group of 4000 C2 landmarks, beyond the 1024-record LDS stage; each at 1024 and 8192 hypotheses, with and without the
local optimisation.  Set B is a similarity (25 degrees, scale 1.3) of set A appended to the map; 30 % of each group's
matches are wrong (the B side moved 100 to 500 map units).  Per row: the median wall time of the call over --repeats
calls after --warmup, and the HIP-event time of its two launches.  For scale, Slam.LocalizeFrames on one C1 frame in
the same session.

    python tools/align_bench.py [--repeats 20] [--warmup 3]
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

import align_cases as ac  # noqa: E402
from slamgpu import ba  # noqa: E402
from slamgpu.scene import make_config  # noqa: E402


def _scene(name, groups_of, share=0.3):
    """(map, groups): B = S_true(A) appended, `share` of each group's matches wrong."""
    m = make_config(name, noise=0.0, outlier_frac=0.0, perturb=False)
    groups_a = groups_of(m)
    used = np.unique(np.concatenate(groups_a)).astype(np.int32)
    b_of = np.full(m.num_points, -1, dtype=np.int32)
    b_of[used] = ac.append_points(m, ac.apply_true(ac.euclid(m, used)))
    # a point of two groups keeps one B side: it is planted, or not, for both
    ac.plant(m, b_of[used], share, 1)
    return m, [np.stack([g, b_of[g]], 1) for g in groups_a]


def _shared(m):
    seen = [set(m.obs_point[m.obs_frame == f]) for f in range(m.num_frames)]
    return [np.array(sorted(seen[f] & seen[f + 1]), dtype=np.int32) for f in range(m.num_frames - 1)]


def _timing(s, what):
    on, ms = getattr(s.lib, "sg_slam_debug_%s_timing" % what), getattr(s.lib, "sg_slam_debug_%s_kernel_ms" % what)
    on.argtypes = [C.c_void_p, C.c_int32]
    ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    return on, ms


def _time(call, s, what, repeats, warmup):
    on, ms = _timing(s, what)
    wall, kern = [], []
    out = None
    for i in range(warmup + repeats):
        if i == warmup:
            on(s.h, 1)
        t0 = time.perf_counter()
        out = call()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            v = C.c_double()
            ms(s.h, C.byref(v))
            wall.append(dt)
            kern.append(v.value)
    return out, {"wall_ms_median": statistics.median(wall), "kernel_ms_median": statistics.median(kern),
                 "wall_ms_min": min(wall), "wall_ms_max": max(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    a = ap.parse_args()
    rows = []
    cases = (("C1, one group of 200", "C1", lambda m: [np.arange(200, dtype=np.int32)]),
             ("C2, 49 groups of shared landmarks", "C2", _shared),
             ("C2, one group of 4000", "C2", lambda m: [np.arange(4000, dtype=np.int32)]))
    for label, name, groups_of in cases:
        m, groups = _scene(name, groups_of)
        for hyp in (1024, 8192):
            for refine in (False, True):
                s = ba.Slam()
                res, t = _time(lambda: s.AlignPoints(m, groups, threshold=ac.TAU, max_hypotheses=hyp, refine=refine), s,
                               "align", a.repeats, a.warmup)
                row = dict(case=label, call="AlignPoints", groups=len(groups),
                           records=int(sum(r["num_records"] for r in res)), hypotheses=hyp, refine=refine,
                           solved=int(sum(r["solved"] for r in res)), **t)
                print(json.dumps(row))
                rows.append(row)
    # for scale: localization of one C1 frame (P3P RANSAC and the pose LM)
    m = make_config("C1", outlier_frac=0.0, perturb=False)
    for hyp in (1024, 8192):
        s = ba.Slam()
        ok, t = _time(lambda: s.LocalizeFrames(m.copy(), [8], max_hypotheses=hyp), s, "pose", a.repeats, a.warmup)
        row = dict(case="C1, frame 8", call="LocalizeFrames", groups=1,
                   records=int(s.localization_results()[0]["num_obs"]), hypotheses=hyp, refine=True, solved=int(sum(ok)),
                   **t)
        print(json.dumps(row))
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/align_bench.py", "repeats": a.repeats, "warmup": a.warmup, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
