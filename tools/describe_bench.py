"""Times sg_tracker_describe (HessianTracker.Describe) on an MI355X and writes profiles/describe_bench.json.

Rows: 120 and 2000 keypoints (seed_points 64 px inside the image, so that every level accepts them) on a 640 x 480
slot, keypoint i on level i % 3.  Per row: the median wall time of the call over --repeats calls after --warmup (the
Python wrapper, the uploads and the downloads included: "per call") and the HIP-event time of its one launch ("per
launch").  For scale, in the same session: sg_tracker_run on the same 2000 points between frames 0 and 1 (7 x 7 window,
3 levels: BASELINE config 3) and sg_hamming_match of the 2000 descriptors of frame 0 against those of frame 1, each
with its wall time and the HIP-event time of its launches.

    python tools/describe_bench.py [--repeats 30] [--warmup 5] [--out profiles/describe_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_amd"))

import numpy as np  # noqa: E402

from slamgpu.matcher import HammingMatcher  # noqa: E402
from slamgpu.tracker import HessianTracker  # noqa: E402
from slamgpu.video import ground_truth, make_frames, seed_points  # noqa: E402


def _stats(wall, kern):
    return {"wall_ms_median": statistics.median(wall), "kernel_ms_median": statistics.median(kern),
            "wall_ms_min": min(wall), "wall_ms_max": max(wall), "kernel_ms_min": min(kern), "kernel_ms_max": max(kern)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "describe_bench.json"))
    a = ap.parse_args()
    frames = make_frames(2)
    t = HessianTracker(window=7, depth=3, max_images=2)
    for s, img in enumerate(frames):
        t.MakePyramid(img, s)
    rows, descs = [], {}
    for n in (120, 2000):
        xy = seed_points(n, border=64.0)
        lv = (np.arange(n) % 3).astype(np.int32)
        wall, kern = [], []
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            desc, ang, st = t.Describe(0, xy, lv)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                wall.append(dt)
                kern.append(t.describe_ms())
        row = dict(case="640 x 480, %d keypoints on levels 0-2" % n, call="sg_tracker_describe", keypoints=n,
                   accepted=int((st == 0).sum()), bins_used=int(len(set(ang[st == 0]))), **_stats(wall, kern))
        print(json.dumps(row))
        rows.append(row)
        if n == 2000:
            descs[0] = desc
            descs[1] = t.Describe(1, ground_truth(xy, 1), lv)[0]
    # for scale: the tracker on the same 2000 points, and all-pairs Hamming on their descriptors
    xy = seed_points(2000, border=64.0)
    wall, kern = [], []
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        t.load_features(xy, xy)
        t.run(0, 1, 1)
        _, acc, _ = t.results()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            wall.append(dt)
            kern.append(t.kernel_ms()[0])
    row = dict(case="640 x 480, 2000 features, 7 x 7 window, 3 levels", call="sg_tracker_run", keypoints=2000,
               accepted=int(acc.sum()), **_stats(wall, kern))
    print(json.dumps(row))
    rows.append(row)
    hm = HammingMatcher(device=0)
    wall, kern = [], []
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        best = hm.match(descs[0], descs[1])[0]
        dt = (time.perf_counter() - t0) * 1e3
        hm.load(descs[0], descs[1])
        hm.run(1)
        ms = hm.results()[3]
        if i >= a.warmup:
            wall.append(dt)
            kern.append(ms)
    hm.close()
    row = dict(case="descriptors of frame 0 against frame 1, 2000 x 2000", call="sg_hamming_match", keypoints=2000,
               own_nearest=int((np.asarray(best) == np.arange(2000)).sum()), **_stats(wall, kern))
    print(json.dumps(row))
    rows.append(row)
    t.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/describe_bench.py", "repeats": a.repeats, "warmup": a.warmup, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
