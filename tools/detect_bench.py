"""Times sg_tracker_detect (HessianTracker.Detect) on an MI355X and writes profiles/detect_bench.json.

Rows: the 640 x 480 texture (frame 0 of make_frames) in a slot of a depth-6 tracker, default thresholds (20/255 and
7/255) and border 15; levels 0..2 and 0..5, per_cell 4 and 8.  Per row: the median wall time of the call over --repeats
calls after --warmup (the Python wrapper, the launch, the copy of the cell slots and the host-side compaction included:
"per call") and the HIP-event time of its one launch ("per launch"), with the keypoints per level.  For scale, in the same
session: sg_tracker_set_image of the same frame (wall, and the HIP-event time of its pyramid kernels),
sg_tracker_seed_features (the Shi-Tomasi seeding of 120 corners; wall only, it records no event time) and
sg_tracker_describe on the keypoints of the levels 0..2, per_cell 4 row (wall and launch).

Not measured: hardware counters, occupancy, LDS bank conflicts; nothing here says where the launch's time goes.

    python tools/detect_bench.py [--repeats 30] [--warmup 5] [--out profiles/detect_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_amd"))

from slamgpu.tracker import HessianTracker  # noqa: E402
from slamgpu.video import make_frames  # noqa: E402


def _stats(wall, kern=None):
    out = {"wall_ms_median": statistics.median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall)}
    if kern is not None:
        out.update({"kernel_ms_median": statistics.median(kern), "kernel_ms_min": min(kern), "kernel_ms_max": max(kern)})
    return out


def _time(a, call, kernel_ms=None):
    wall, kern, last = [], [], None
    for i in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        last = call()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            wall.append(dt)
            if kernel_ms:
                kern.append(kernel_ms())
    return last, _stats(wall, kern if kernel_ms else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_bench.json"))
    a = ap.parse_args()
    img = make_frames(1)[0]
    t = HessianTracker(window=13, depth=6, max_images=2)
    t.MakePyramid(img, 0)
    rows, keypoints = [], None
    for num_levels in (3, 6):
        for per_cell in (4, 8):
            (xy, lv, sc, per), st = _time(a, lambda: t.Detect(0, num_levels=num_levels, per_cell=per_cell), t.detect_ms)
            row = dict(case="640 x 480, levels 0-%d, per_cell %d" % (num_levels - 1, per_cell), call="sg_tracker_detect",
                       keypoints=len(xy), cells=sum(p["cells"] for p in per),
                       candidates=[p["candidates"] for p in per[:num_levels]],
                       low_cells=[p["low_cells"] for p in per[:num_levels]],
                       keypoints_per_level=[p["keypoints"] for p in per[:num_levels]], **st)
            print(json.dumps(row))
            rows.append(row)
            if num_levels == 3 and per_cell == 4:
                keypoints = (xy, lv)
    # for scale, in the same session
    _, st = _time(a, lambda: t.MakePyramid(img, 1), lambda: t.kernel_ms()[1])
    rows.append(dict(case="640 x 480, depth 6", call="sg_tracker_set_image", **st))
    print(json.dumps(rows[-1]))
    (corners, _), st = _time(a, lambda: t.SeedFeatures(0))
    rows.append(dict(case="640 x 480, 120 corners, min distance 20", call="sg_tracker_seed_features",
                     keypoints=len(corners), **st))
    print(json.dumps(rows[-1]))
    (desc, ang, status), st = _time(a, lambda: t.Describe(0, *keypoints), t.describe_ms)
    rows.append(dict(case="the keypoints of the levels 0-2, per_cell 4 row", call="sg_tracker_describe",
                     keypoints=len(keypoints[0]), accepted=int((status == 0).sum()), **st))
    print(json.dumps(rows[-1]))
    t.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/detect_bench.py", "repeats": a.repeats, "warmup": a.warmup,
                   "not_measured": "hardware counters, occupancy, LDS bank conflicts", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
