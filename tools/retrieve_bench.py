"""Times keyframe retrieval (HammingMatcher.query_keyframes, sg_matcher_db_query) on an MI355X and writes
profiles/retrieve_bench.json.

Rows: databases of 50 and 200 keyframes of 2000 descriptors each, queries of 500 and 2000 descriptors.  One keyframe is
A of make_descriptor_sets(2000, seed=5) and the query the first rows of its B (70 % noisy copies, 30 % fresh rows); the
other keyframes are random.  Per row: the median wall time of the one call over --repeats calls after --warmup (the
Python wrapper, the query's upload and the download of the best set's rows included), and the HIP-event time of its
launches.  In the same session, the thing the call replaces: a loop of sg_hamming_match over the same keyframes (two
uploads, two launches and a synchronisation each) with the acceptance and one-to-one rules in numpy on the host; its
scores are checked equal to the call's.

    python tools/retrieve_bench.py [--repeats 30] [--warmup 3]
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

from slamgpu.matcher import HammingMatcher, make_descriptor_sets  # noqa: E402

MAX_DIST, RATIO = 64, 80


def host_rules(bi, bd, sd):
    """Acceptance and the one-to-one rule on one set's (best_idx, best_dist, second_dist): the score."""
    cand = np.flatnonzero((bi >= 0) & (bd <= MAX_DIST) & ((sd < 0) | (100 * bd <= RATIO * sd)))
    order = cand[np.lexsort((cand, bd[cand]))]            # by (distance, query index)
    return len(np.unique(bi[order]))                      # one winner per claimed descriptor


def loop_of_matches(hm, sets, q):
    return np.array([host_rules(*hm.match(q, t)) for t in sets], np.int32)


def median_ms(call, repeats, warmup, after=None):
    wall, extra = [], []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        call()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            wall.append(dt)
            if after:
                extra.append(after())
    return wall, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieve_bench.json"))
    a = ap.parse_args()
    A, B, _ = make_descriptor_sets(2000, seed=5)
    rng = np.random.default_rng(50)
    rows = []
    for S in (50, 200):
        sets = [A if s == S // 2 else rng.integers(0, 2 ** 64, (2000, 4), dtype=np.uint64, endpoint=False)
                for s in range(S)]
        hm = HammingMatcher(device=0)
        t0 = time.perf_counter()
        for t in sets:
            hm.add_keyframe(t)
        add_ms = (time.perf_counter() - t0) * 1e3
        for nq in (500, 2000):
            q = np.ascontiguousarray(B[:nq])
            wall, kern = median_ms(lambda: hm.query_keyframes(q, k=1), a.repeats, a.warmup, hm.query_keyframes_ms)
            score, top_set, top_score, _, _ = hm.query_keyframes(q, k=1)
            loop_wall, _ = median_ms(lambda: loop_of_matches(hm, sets, q), a.repeats, a.warmup)
            same = bool((loop_of_matches(hm, sets, q) == score).all())
            row = dict(sets=S, descriptors_per_set=2000, queries=nq, pairs=S * 2000 * nq,
                       call_wall_ms_median=statistics.median(wall), call_wall_ms_min=min(wall),
                       call_wall_ms_max=max(wall), launches_ms_median=statistics.median(kern),
                       loop_wall_ms_median=statistics.median(loop_wall), loop_wall_ms_min=min(loop_wall),
                       loop_wall_ms_max=max(loop_wall), loop_scores_equal=same, best_set=int(top_set[0]),
                       best_score=int(top_score[0]), add_all_sets_ms=add_ms)
            print(json.dumps(row), flush=True)
            rows.append(row)
        hm.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/retrieve_bench.py", "repeats": a.repeats, "warmup": a.warmup, "rows": rows}, f,
                  indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
