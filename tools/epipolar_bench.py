"""Times sg_slam_match_epipolar (Slam.MatchEpipolar) on an MI355X and writes profiles/epipolar_bench.json.

Rows: one stereo pair of C2 with 500 keypoints a side; one with 2000 a side; ten pairs of 2000 a side in one call; and
the ten pairs as ten single-pair calls.  Keypoints as in tests/epipolar_cases.py: the frame's observation pixels with
the landmark's descriptor after Binomial(256, 0.03) bit flips, a quarter as many distractors, random levels 0..3,
shuffled, cut to the row's count; default options (a 2 px gate, no parallax test).  Per row: the median wall time of
the call over --repeats calls after --warmup (the Python wrapper included) and the HIP-event time of its three
launches.  Beside them, in the same session: the all-pairs sg_hamming_match on the same descriptor counts (wall and
the HIP-event time of its two launches), and the planner's CPU executor on one host thread (the library's diagnostic
entry point; wall time, no device).

    python tools/epipolar_bench.py [--repeats 30] [--warmup 3]
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

import epipolar_cases as ec  # noqa: E402
import match_cases as mc  # noqa: E402
from slamgpu import ba  # noqa: E402
from slamgpu.matcher import HammingMatcher  # noqa: E402
from slamgpu.scene import make_config  # noqa: E402


def _median_times(call, s, repeats, warmup):
    on, ms = s.lib.sg_slam_debug_epipolar_timing, s.lib.sg_slam_debug_epipolar_kernel_ms
    on.argtypes = [C.c_void_p, C.c_int32]
    ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    wall, kern = [], []
    for i in range(warmup + repeats):
        if i == warmup:
            on(s.h, 1)
        t0 = time.perf_counter()
        kernel = call(lambda: _kernel_ms(ms, s))
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
            kern.append(kernel)
    return {"wall_ms_median": statistics.median(wall), "kernel_ms_median": statistics.median(kern),
            "wall_ms_min": min(wall), "wall_ms_max": max(wall)}


def _kernel_ms(ms, s):
    v = C.c_double()
    ms(s.h, C.byref(v))
    return v.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epipolar_bench.json"))
    a = ap.parse_args()
    m = make_config("C2", noise=0.0, outlier_frac=0.0, perturb=False)
    desc = mc._random_desc(np.random.default_rng(8), m.num_points)

    def side(f, count):
        nobs = int((m.obs_frame == f).sum())
        kp = ec.frame_keypoints(m, desc, f, 5000 + f, distract=nobs // 4)
        assert len(kp[0]) >= count, (f, len(kp[0]))
        return tuple(x[:count] for x in kp[:3])

    rows = []
    ten = [(20 + 2 * i, 21 + 2 * i) for i in range(10)]   # (the first frames of C2 see too few points)
    cases = (("one pair, 500 x 500", ten[:1], 500, False), ("one pair, 2000 x 2000", ten[:1], 2000, False),
             ("ten pairs of 2000 x 2000, one call", ten, 2000, False),
             ("ten pairs of 2000 x 2000, ten calls", ten, 2000, True))
    for label, pairs, count, split in cases:
        ka, kb = [side(p[0], count) for p in pairs], [side(p[1], count) for p in pairs]
        s = ba.Slam()

        def call(kernel_ms, s=s, pairs=pairs, ka=ka, kb=kb, split=split):
            if not split:
                s.MatchEpipolar(m, pairs, ka, kb)
                return kernel_ms()
            total = 0.0
            for i in range(len(pairs)):
                s.MatchEpipolar(m, pairs[i:i + 1], ka[i:i + 1], kb[i:i + 1])
                total += kernel_ms()
            return total

        t = _median_times(call, s, a.repeats, a.warmup)
        s.MatchEpipolar(m, pairs, ka, kb)
        res = s.epipolar_match_results()
        nc = np.concatenate([r["num_candidates"] for r in res])
        row = dict(case=label, call="MatchEpipolar", pairs=len(pairs), keypoints_a=count * len(pairs),
                   keypoints_b=count * len(pairs), mean_candidates=float(nc.mean()),
                   matched=int(sum(r["num_matched"] for r in res)), **t)
        print(json.dumps(row))
        rows.append(row)
        if not split:
            # the planner's CPU executor on one host thread, same call
            wall = []
            for i in range(min(a.repeats, 10)):
                t0 = time.perf_counter()
                cpu = ba.match_epipolar_cpu(m, pairs, ka, kb)
                wall.append((time.perf_counter() - t0) * 1e3)
            assert all(np.array_equal(x["match"], y["match"]) for x, y in zip(cpu, res))
            row = dict(case=label, call="CPU executor, one thread", pairs=len(pairs), keypoints_a=count * len(pairs),
                       keypoints_b=count * len(pairs), wall_ms_median=statistics.median(wall), wall_ms_min=min(wall),
                       wall_ms_max=max(wall))
            print(json.dumps(row))
            rows.append(row)
    # for scale: all-pairs Hamming on the same descriptor counts
    for count in (500, 2000):
        qd, td = side(ten[0][0], count)[1], side(ten[0][1], count)[1]
        hm = HammingMatcher(device=0)
        wall, kern = [], []
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            hm.match(qd, td)
            dt = (time.perf_counter() - t0) * 1e3
            hm.load(qd, td)
            hm.run(1)
            ms = hm.results()[3]
            if i >= a.warmup:
                wall.append(dt)
                kern.append(ms)
        hm.close()
        row = dict(case="descriptors alone, %d x %d" % (count, count), call="sg_hamming_match", pairs=1,
                   keypoints_a=count, keypoints_b=count, wall_ms_median=statistics.median(wall),
                   kernel_ms_median=statistics.median(kern), wall_ms_min=min(wall), wall_ms_max=max(wall))
        print(json.dumps(row))
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/epipolar_bench.py", "repeats": a.repeats, "warmup": a.warmup, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
