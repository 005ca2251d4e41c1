"""Times sg_slam_relative_poses (Slam.RelativePoses) on an MI355X and writes profiles/relpose_bench.json.

Rows: one C1 pair (the stereo pair (4, 5), 211 records) and the consecutive pairs of C2 (49 pairs), at 1024 and 8192
hypotheses, with and without the local optimisation.  Per row: the median wall time of the call over --repeats calls
after --warmup, and the HIP-event time of its two launches.  30 % of each pair's records are planted outliers.

    python tools/relpose_bench.py [--repeats 20] [--warmup 3]
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

from slamgpu import ba  # noqa: E402
from slamgpu.scene import HEIGHT, WIDTH, make_config  # noqa: E402


def _scene(name, pairs, share=0.3):
    m = make_config(name, outlier_frac=0.0, perturb=False)
    rng = np.random.default_rng(1)
    pts = m.obs_pt.reshape(-1, 2)
    for _, b in pairs:   # uniform pixels: a few land near the epipolar line, which a benchmark does not mind
        sel = np.flatnonzero(m.obs_frame == b)
        bad = rng.choice(sel, size=int(share * len(sel)), replace=False)
        pts[bad] = rng.uniform((0.0, 0.0), (WIDTH, HEIGHT), size=(len(bad), 2))
    return m


def _time(m, pairs, hyp, refine, repeats, warmup):
    s = ba.Slam()
    s.lib.sg_slam_debug_relpose_timing.argtypes = [C.c_void_p, C.c_int32]
    s.lib.sg_slam_debug_relpose_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    wall, kern = [], []
    ok = None
    for i in range(warmup + repeats):
        if i == warmup:
            s.lib.sg_slam_debug_relpose_timing(s.h, 1)
        t0 = time.perf_counter()
        ok = s.RelativePoses(m, pairs, max_hypotheses=hyp, refine=refine)
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            ms = C.c_double()
            s.lib.sg_slam_debug_relpose_kernel_ms(s.h, C.byref(ms))
            wall.append(dt)
            kern.append(ms.value)
    res = s.relative_pose_results()
    return {"pairs": len(pairs), "records": int(sum(r["num_obs"] for r in res)), "hypotheses": hyp, "refine": refine,
            "solved": int(sum(ok)), "wall_ms_median": statistics.median(wall), "kernel_ms_median": statistics.median(kern),
            "wall_ms_min": min(wall), "wall_ms_max": max(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relpose_bench.json"))
    a = ap.parse_args()
    rows = []
    for name, pairs in (("C1", [(4, 5)]), ("C2", [(f, f + 1) for f in range(49)])):
        m = _scene(name, pairs)
        for hyp in (1024, 8192):
            for refine in (False, True):
                row = dict(config=name, **_time(m, pairs, hyp, refine, a.repeats, a.warmup))
                print(json.dumps(row))
                rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/relpose_bench.py", "repeats": a.repeats, "warmup": a.warmup, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
