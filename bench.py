#!/usr/bin/env python3
"""Benchmark: local bundle-adjustment LM iterations/sec on MI355X (BASELINE.json metric).

One "step" = one Levenberg-Marquardt iteration of the reference's local BA (slam.cpp:482-521, Ceres 1.8
LM + SPARSE_SCHUR restated on the GPU): linearize (if the previous step was accepted), damp + Schur
complement, reduced camera Cholesky, back-substitution, candidate cost, accept/reject — all on device.

Workloads (synthetic scenes, slamgpu/scene.py; fp64 arithmetic, the reference's own precision):
  --config C2 (default): BASELINE config 2 — 50 keyframes / ~19.4k landmarks / ~148k observations (seed 2),
      SolveFrames(map, 48, 50, 2.0).  N > 1 (torchrun, one rank per GPU): strong scaling — the same 20k-landmark
      problem's landmarks sharded over the ranks (sg_problem_shard), RCCL all-reduces of the camera system per
      iteration; value = K / time.  The weak-scaling figure (50 keyframes and N x 20k landmarks, value =
      N * K / time in units of config-2 iterations) is reported beside it as `weak_scaling`.
  --config C5: BASELINE config 5 — 200 keyframes / ~194k landmarks / ~1.95M observations (seed 5),
      SolveFrames(map, 198, 200, 2.0); N > 1: strong scaling, the same problem's landmarks sharded over the
      ranks; value = K / time.
A plain run (`--gpus N --steps K --warmup W`) does what the headline figure needs and no more: it builds the
workload, warms up, times the K steps, writes the outputs if `--dump-outputs DIR` is given, and prints the line;
the fields of the other measurements are null in it.  `--full` adds everything described below: the per-kernel
and `lm_regime` passes, `solve_from_start`, the other workload (C5 next to a C2 headline: strong over the same N
ranks), the scaled sweep, SolveAllFrames, the scaling model, the CPU baselines and the front end.

`--dump-outputs DIR` writes what the K-th timed iteration left, as a caller of the solver receives it
(sg_ba_download): DIR/q.npy (frames x 4), t.npy (frames x 3), X.npy (landmarks x 4) and cost.npy, float64 (and
k.npy when the intrinsics are free).  The scene generator is seeded, so the inputs are the same from run to run.

The timed region is K LM iterations with termination disabled after W warm-up iterations, and every
iteration is SURVEY.md 8d's full unit of work: linearize + Schur + Cholesky + back-substitution + candidate
cost + decision.  Ceres skips the linearization after a rejected step; the benchmark re-linearizes there too
(sg_solver_options.always_linearize: the same values, so the same trajectory), so value and ms_per_step do
not depend on K, W or how many steps past convergence get rejected.  `lm_regime` times the same K with
Ceres's own skipping (its share of accepted steps depends on K), and `solve_from_start` times complete solves
from the perturbed start (Slam::SolveFrames semantics, termination on): iterations / wall time.

Roofline `traffic` fields come from the per-workload rocprofv3 --pmc passes (tools/profile_round.sh ->
profiles/<tag>_pmc_traffic_<workload>.json, newest tag wins), run with `--only <workload>` so each file holds
that workload's own launches; `--only` also serves the per-workload kernel-trace profiles.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "slam-robot_amd"))

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E peak (MI355X_MICROARCH.md)
FP64_PEAK_TFLOPS = 78.6      # MI355X FP64 vector / matrix peak


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--points", type=int, default=20000, help="landmarks of the config-2 scene")
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--config", choices=("C2", "C5"), default="C2", help="headline workload")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline figure, measure everything else: the per-kernel and Ceres-regime "
                         "passes, solves from the start, the other workload, the scaled sweep, SolveAllFrames, the "
                         "scaling model, the CPU baselines and the front end (each has its own switch below); "
                         "--only implies it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one left (poses q, t, landmarks X, the cost) "
                         "as DIR/<name>.npy (float64)")
    ap.add_argument("--other", type=int, default=1, help="also measure the other BA workload (C5 / C2)")
    ap.add_argument("--cpu-runs", type=int, default=7, help="CPU-baseline timed runs per leg (0: skip)")
    ap.add_argument("--cpu-seconds", type=float, default=4.0, help="front-end CPU-baseline sample (0: skip)")
    ap.add_argument("--sweep-obs", type=int, default=2_000_000,
                    help="observations in the scaled Jacobian-sweep measurement (0: skip)")
    ap.add_argument("--frontend", type=int, default=1,
                    help="also measure the front end at N=1: KLT tracks/sec (config 3) and the 256-bit "
                         "Hamming matcher (config 4)")
    ap.add_argument("--solve-all", type=int, default=1,
                    help="N = 1: also time SolveAllFrames(C2 map, 2, false/true) (whole map; dense with cameras)")
    ap.add_argument("--model-scaling", type=int, default=1,
                    help="N = 1: model C2 and C5 strong scaling over 2/4/8 landmark shards from measured kernel "
                         "times")
    ap.add_argument("--weak", type=int, default=1,
                    help="N > 1: also measure C2 weak scaling (N x 20k landmarks) beside the strong headline")
    ap.add_argument("--comm", choices=("rccl", "host"), default="rccl",
                    help="N > 1: rccl (one GPU per rank, the product path) or host (torch.distributed gloo through "
                         "sg_ba_comm_init_host: rehearses the multi-rank bench with several ranks on one GPU)")
    ap.add_argument("--only", choices=("all", "C2", "C5", "sweep", "frontend"), default="all",
                    help="profiling runs: one workload alone (its kernels are then the only ones launched)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.only != "all":
        args.full = True
    if not args.full:   # a plain run: set up, warm up, time the K steps, print the line
        args.other = args.cpu_runs = args.sweep_obs = args.frontend = args.solve_all = 0
        args.model_scaling = args.weak = 0
        args.cpu_seconds = 0.0
    if args.only != "all":
        args.solve_all = 0
        args.cpu_runs = 0
        args.cpu_seconds = 0
        args.other = 0
        args.frontend = 1 if args.only == "frontend" else 0
        args.sweep_obs = args.sweep_obs if args.only == "sweep" else 0
        if args.only in ("C2", "C5"):
            args.config = args.only
    return args


FP32_PEAK_TFLOPS = 157.3     # MI355X FP32 vector peak
I8_MFMA_PEAK_TOPS = 5033.0    # int8 MFMA (dense): 2048 ops/clk/SIMD (16x16x64 in 16 cycles) x 1024 SIMDs x 2.4 GHz


def pmc_traffic(kernel, workload):
    """HBM bytes per launch of `kernel` in `workload` (C2, C5, sweep, frontend) from the committed
    rocprofv3 FETCH_SIZE / WRITE_SIZE passes of `bench.py --only <workload>` (tools/profile_round.sh ->
    profiles/r<round>_v<version>_pmc_traffic_<workload>.json, newest version wins).  Each file holds one
    workload's launches only, so the figure is that workload's own kernel; returns (bytes, file) or
    (None, None)."""
    import glob
    import re

    def order(f):   # r<round>_v<version>: numeric, so r3_v12 comes after r3_v5
        m = re.match(r"r(\d+)_v(\d+)_", os.path.basename(f))
        return (int(m.group(1)), int(m.group(2))) if m else (0, 0)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic_%s.json" % workload)), key=order)
    if not files:
        return None, None
    groups = [g for g in json.load(open(files[-1]))["kernels"].values() if g["kernel"] == kernel]
    if not groups:
        return None, os.path.basename(files[-1])
    g = max(groups, key=lambda g: g["active_dispatches"])
    return g["traffic_bytes"], os.path.basename(files[-1])


def pmc_mfma(kernel, workload):
    """Matrix-core counters per launch of `kernel` in `workload` (C2, C5) from the committed rocprofv3 pass of
    SQ_VALU_MFMA_BUSY_CYCLES / GRBM_GUI_ACTIVE over `bench.py --only <workload>` (tools/profile_round.sh ->
    profiles/r<round>_v<version>_pmc_mfma_<workload>.json, tools/pmc_mfma.py; newest version wins)."""
    import glob
    import re

    def order(f):
        m = re.match(r"r(\d+)_v(\d+)_", os.path.basename(f))
        return (int(m.group(1)), int(m.group(2))) if m else (0, 0)
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_mfma_%s.json" % workload)), key=order)
    if not files:
        return None
    groups = [g for g in json.load(open(files[-1]))["kernels"].values() if g["kernel"] == kernel]
    if not groups:
        return None
    g = max(groups, key=lambda g: g["dispatches"])
    busy = g.get("mfma_busy_cycles_per_launch", 64.0 * g.get("mfma_per_launch", 0.0))   # (r4/r5_v6 files: count)
    return {"mfma_busy_frac": g["mfma_busy_frac"], "mfma_busy_cycles_per_launch": busy,
            "pmc_file": os.path.basename(files[-1])}


TRAFFIC_APPLIES = True   # False for N > 1: the committed PMC files profile the one-GPU workload, not a shard


def traffic_fields(kernel, workload, algorithmic_bytes=None):
    if not TRAFFIC_APPLIES:
        return {"traffic": None, "traffic_file": None}
    t, src = pmc_traffic(kernel, workload)
    d = {"traffic": t, "traffic_file": src}
    if t is not None and algorithmic_bytes:
        d["traffic_over_algorithmic"] = t / algorithmic_bytes
    return d


def bench_tracker(local, cpu_seconds):
    """BASELINE config 3: 640x480 synthetic video, 2000 tracks, 3-level pyramid, 7x7 window, forward/backward
    TrackFeature (matcher.cpp:173-206).  Inputs resident on the device; value = tracks / kernel time."""
    from slamgpu.tracker import HessianTracker
    from slamgpu.video import make_frames, seed_points
    frames = make_frames(2)
    pts = seed_points(2000)
    W, depth, reps = 7, 3, 50
    t = HessianTracker(window=W, depth=depth, device=local, retry_levels=0)
    t.MakePyramid(frames[0], 0)
    t.MakePyramid(frames[1], 1)
    _, pyr_ms = t.kernel_ms()
    t.load_features(pts, pts)
    t.run(0, 1, 3)
    t.results()
    t.run(0, 1, reps)
    out, acc, its = t.results()
    track_ms, _ = t.kernel_ms()
    ms = track_ms / reps
    value = len(pts) / (ms * 1e-3)
    flops = float(its.sum()) * 108.0 * W * W        # 108 W^2 flops per Newton iteration
    ach = flops / (ms * 1e-3) / 1e12
    res = {"metric": "KLT tracks/sec (640x480, 2000 tracks, 3 levels, 7x7, forward+backward)",
           "value": value, "unit": "tracks/s", "ms_per_frame_tracking": ms, "ms_pyramid": pyr_ms,
           "tracks_per_s_with_pyramid": len(pts) / ((ms + pyr_ms) * 1e-3),
           "accepted_frac": float(acc.mean()), "newton_iterations": int(its.sum()),
           # one wave per track and ~2 waves per SIMD: the launch lasts as long as its longest serial
           # Newton chain, so the per-iteration latency of that chain is the number that bounds the kernel
           "newton_iterations_max_track": int(its.max()),
           "us_per_newton_iteration_on_longest_track": ms * 1e3 / max(int(its.max()), 1),
           "roofline": {"bound": "valu", "achieved": ach, "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": ach / FP32_PEAK_TFLOPS, **traffic_fields("k_track_fb", "frontend"), "kernel": "k_track_fb",
                        "note": "108*W^2 flops per Newton iteration (6 probes of bilinear sampling, moments, "
                                "score); one wave per feature"}}
    if cpu_seconds > 0:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle
        pf, dims = oracle.make_pyramid(frames[0], depth)
        pt, _ = oracle.make_pyramid(frames[1], depth)
        threads = min(16, os.cpu_count() or 1)
        done, tc = 0, 0.0
        while tc < cpu_seconds:
            tt = time.perf_counter()
            oracle.track_fb(pf, pt, dims, W, pts, pts, np.full(len(pts), depth, np.int32), nthreads=threads,
                            retry_levels=0)
            tc += time.perf_counter() - tt
            done += len(pts)
        res["cpu_baseline"] = {"value": done / tc, "unit": "tracks/s", "cores": threads, "kind": "port",
                               "sample": "%d forward/backward tracks (oracle/oracle_track.cpp, OpenMP over "
                                         "tracks) in %.1f s" % (done, tc)}
    return res


def bench_hamming(local, cpu_seconds):
    """BASELINE config 4: 10k x 10k 256-bit descriptors, all pairs, best + second-best per query."""
    from slamgpu.matcher import HammingMatcher, make_descriptor_sets
    A, B, truth = make_descriptor_sets(10000)
    m = HammingMatcher(device=local)
    m.load(B, A)
    m.run(3)
    m.results()
    reps = 20
    m.run(reps)
    bi, bd, sd, ms = m.results()
    pairs = float(len(A)) * len(B)
    ops = pairs * 512.0      # per pair: a 256-term int8 dot product (256 multiply-adds) on the matrix cores
    ach = ops / (ms * 1e-3) / 1e12
    alg_ops = pairs * 12.0   # 4 XOR + 4 POPC + 3 ADD + 1 MIN per pair (the algorithm's count)
    res = {"metric": "256-bit Hamming all-pairs query-rows/sec (10k x 10k)", "value": len(B) / (ms * 1e-3),
           "unit": "rows/s", "pairs_per_s": pairs / (ms * 1e-3), "ms": ms,
           "recall_of_true_matches": float((bi[truth >= 0] == truth[truth >= 0]).mean()),
           "roofline": {"bound": "mfma", "achieved": ach, "peak": I8_MFMA_PEAK_TOPS, "unit": "TOPS (int8)",
                        "frac": ach / I8_MFMA_PEAK_TOPS, **traffic_fields("k_hamming_slices", "frontend"),
                        "kernel": "k_hamming_slices",
                        "algorithmic_int_ops_per_s": alg_ops / (ms * 1e-3),
                        "algorithmic_note": "SURVEY.md 8d prices the algorithm at 12 integer ops per pair "
                                            "(XOR/POPC/ADD/MIN on 4 x u64); the frac above prices the "
                                            "implementation's 512 int8 MFMA ops per pair",
                        "note": "+-1 int8 dot products (v_mfma_i32_16x16x64_i8, 2 x 256 ops per pair) with the "
                                "expansion and the arg-min fused; whole match (slices + merge) per HIP-event time"}}
    if cpu_seconds > 0:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle
        threads = min(16, os.cpu_count() or 1)
        done, tc = 0, 0.0
        while tc < cpu_seconds:
            tt = time.perf_counter()
            oracle.hamming_match(B, A, nthreads=threads)
            tc += time.perf_counter() - tt
            done += len(B)
        res["cpu_baseline"] = {"value": done / tc, "unit": "rows/s", "cores": threads, "kind": "port",
                               "sample": "%d query rows x 10k (oracle, popcnt, OpenMP) in %.1f s" % (done, tc)}
    return res


def bench_matcher_sequence(local, cpu):
    """Matcher::Track per frame (matcher.cpp:301-405) over the 11-frame sequence the front-end parity test uses
    (slamgpu.video.matcher_sequence: 320x240, 13x13 window, 6-level pyramid; seeding, tracking frames, scene
    cuts, view expiry): the device front end (pyramid, FindMatches as one launch per pass, corner seeding, the
    bookkeeping in host C++, the map through Python callbacks) timed per Track call after one warm-up pass of
    the whole sequence, beside the sequential restatement (oracle/oracle_matcher.py over the C++ tracker
    oracle) on the same frames."""
    import statistics
    from slamgpu.frontend import Matcher, add_frame
    from slamgpu.scene import MapArrays
    from slamgpu.video import SEQ_K, matcher_sequence, sequence_mark, sequence_pose, sequence_true_t
    frames, _ = matcher_sequence()

    def run():
        z = lambda dt: np.zeros(0, dt)  # noqa: E731
        m = MapArrays(k=SEQ_K.copy(), q=z(np.float64), t=z(np.float64), frame_camera=z(np.int32),
                      frame_prev=z(np.int32), X=z(np.float64), point_flags=z(np.int32),
                      point_uncertainty=z(np.float64), obs_pt=z(np.float64), obs_frame=z(np.int32),
                      obs_point=z(np.int32), obs_disabled=z(np.int32), obs_error=z(np.float64),
                      frame_keyframe=z(np.int32))
        mt = Matcher(device=local, window=13, depth=6)
        ms, batches, stats = [], [], []
        for i, img in enumerate(frames):
            q, t = sequence_pose(i)
            add_frame(m, 0, q, t)
            sequence_mark(i, m.point_flags, m.point_uncertainty, m.num_points)

            def upd(i=i):
                m.t[3 * i:3 * i + 3] = sequence_true_t(i)
                return i % 2 == 1
            t0 = time.perf_counter()
            mt.Track(img, i, 0, m, upd)
            ms.append(1e3 * (time.perf_counter() - t0))
            batches.append(mt.last_stats["track_batches"])
            stats.append((mt.last_stats["matches"], mt.last_stats["keyframe"]))
        mt.close()
        return ms, batches, stats

    run()
    ms, batches, stats = run()
    res = {"metric": "Matcher::Track ms per frame (11-frame sequence, 320x240, 13x13, 6 levels)",
           "ms_per_frame_median": statistics.median(ms), "ms_per_frame_mean": sum(ms) / len(ms),
           "ms_per_frame": [round(x, 3) for x in ms], "track_launches_per_frame": batches,
           "matches_keyframe": stats,
           "note": "wall time of sg_frontend_track through the Python mirror (map callbacks in Python): pyramid, "
                   "FindMatches (one k_find_matches launch per pass: a wave per feature walks its views), corner "
                   "seeding on keyframes, bookkeeping"}
    if cpu:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import oracle_matcher as om
        omap = om.OracleMap(SEQ_K, [], [], [])
        mt = om.OracleMatcher()
        oms = []
        for i, img in enumerate(frames):
            q, t = sequence_pose(i)
            omap.q.append(list(q))
            omap.t.append(list(t))
            omap.frame_camera.append(0)
            omap.obs[i] = []
            omap.keyframe.append(0)
            sequence_mark(i, omap.flags, omap.uncertainty, len(omap.X))

            def oupd(i=i):
                omap.t[i] = list(sequence_true_t(i))
                return i % 2 == 1
            t0 = time.perf_counter()
            mt.Track(img, i, omap, oupd)
            oms.append(1e3 * (time.perf_counter() - t0))
        res["cpu_baseline"] = {"value": statistics.median(oms), "unit": "ms/frame (median)", "cores": 1,
                               "kind": "port", "ms_per_frame": [round(x, 2) for x in oms],
                               "sample": "oracle/oracle_matcher.py (features one at a time, C++ tracker oracle) "
                                         "over the same 11 frames"}
    return res


def dist_env():
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    return ws, rank, local


def cpu_legs(full, runs, ba_iters_note):
    """CPU baseline of one LM iteration (oracle/oracle_ba.cpp, the Ceres-1.8 LM + SPARSE_SCHUR restatement).
    A solve from the perturbed start with max_num_iterations = k pays the set-up, iteration 0's residual and
    Jacobian pass and k LM iterations; one LM iteration is timed as the difference T(2) - T(1) of the medians of
    `runs` timed runs each (1 warm-up run each; both accepted steps on this problem, so each iteration
    linearizes — the same unit as the device figure).  Legs: 1 thread (the reference's Ceres num_threads
    default, slam.cpp:504), 1 thread with -ffast-math (the reference's Makefile:4 flags), and this process's CPU
    share on OpenMP."""
    import statistics
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    from slamgpu.capi import default_solver_options
    nproc = os.cpu_count() or 1
    affinity = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else nproc
    share = min(affinity, int(os.environ.get("OMP_NUM_THREADS", affinity)))
    legs = []
    def iqr(ts):
        q = statistics.quantiles(ts, n=4) if len(ts) >= 2 else [ts[0]] * 3
        return q[2] - q[0]

    # 1 thread (the reference's setting) and OpenMP on all host cores.  The all-cores leg sets its
    # thread count explicitly (the affinity count, whatever OMP_NUM_THREADS says); the OMP_NUM_THREADS share (the
    # box's CPU share for one GPU) is timed beside it when it differs.
    spec = [("1 thread, -O3", 1, False), ("1 thread, -O3 -ffast-math", 1, True)]
    allc = min(affinity, 256)   # (bounded: the box's task limit)
    if share != allc:
        spec.append(("%d threads (OpenMP, OMP_NUM_THREADS share), -O3" % share, share, False))
    spec.append(("%d threads (OpenMP, all cores in the affinity mask), -O3" % allc, allc, False))
    for name, nt, fm in spec:
        n_runs, noisy, attempts = runs, True, 3
        for attempt in range(attempts):   # the difference of two medians must clear their spread, else time more runs
            med, spread = {}, {}
            for k in (1, 2):
                o = default_solver_options(max_num_iterations=k)
                ts = []
                for r in range(1 + n_runs):
                    po = full.copy()
                    t0 = time.perf_counter()
                    s = oracle.solve(po, o, nthreads=nt, fastmath=fm)
                    if r >= 1:
                        ts.append(time.perf_counter() - t0)
                assert s["num_successful_steps"] == k, s
                med[k], spread[k] = statistics.median(ts), iqr(ts)
            per_it = med[2] - med[1]
            if per_it > spread[1] + spread[2]:
                noisy = False
                break
            if attempt + 1 < attempts:   # `runs` reports the count actually timed
                n_runs *= 2
        # a leg whose T(2) - T(1) never turns positive is reported invalid, not fatal to the GPU line
        ok = per_it > 0
        legs.append({"leg": name, "threads": nt, "fastmath": fm, "value": 1.0 / per_it if ok else None,
                     "unit": "iters/s", "s_per_iteration": per_it if ok else None,
                     "median_s_1_iteration_solve": med[1],
                     "median_s_2_iteration_solve": med[2], "iqr_s_1_iteration_solve": spread[1],
                     "iqr_s_2_iteration_solve": spread[2], "runs": n_runs,
                     "noisy": noisy or not ok})
    valid = [l for l in legs if l["value"] is not None]
    best = max(valid, key=lambda l: l["value"]) if valid else {"value": None, "threads": None}
    return {"value": best["value"], "unit": "iters/s", "cores": best["threads"], "kind": "port",
            "sample": "one LM iteration = T(2 iterations) - T(1 iteration), medians of >= %d runs each: "
                      "SolveFrames(%s) from the perturbed start (oracle/oracle_ba.cpp, dual-number Jacobians); "
                      "nproc=%d, affinity %d, OMP_NUM_THREADS share %d; value = the best leg" % (
                          runs, ba_iters_note, nproc, affinity, share),
            "nproc": nproc, "affinity_share": affinity, "omp_share": share, "legs": legs}


def make_workload(cfg, n_gpus, rank, points, frames, weak=False):
    """(full problem, this rank's shard, description) of a BA workload.  C2 is the `points`-landmark problem
    sharded over the ranks (strong scaling); weak=True builds n_gpus x `points` landmarks instead."""
    from slamgpu import ba
    from slamgpu.scene import make_config, make_scene
    if cfg == "C2":
        npts = points * n_gpus if weak else points
        scene = make_scene(num_frames=frames, num_points=npts, seed=2, run_max=14, run_min=4)
        full = ba.problem_from_map_frames(scene, frames - 2, frames, 2.0)
        desc = "config 2: SolveFrames(%d of %d KF) local BA, LM iteration%s" % (
            frames - 2, frames, " (weak scaling: %d x %d landmarks)" % (n_gpus, points) if weak else "")
    else:
        scene = make_config("C5")
        full = ba.problem_from_map_frames(scene, scene.num_frames - 2, scene.num_frames, 2.0)
        desc = "config 5: SolveFrames(198 of 200 KF) local BA, LM iteration"
    prob = ba.shard_problem(full, rank, n_gpus) if n_gpus > 1 else full
    return full, prob, desc


class Runner:
    """One BA workload on this rank: its solver (and RCCL communicator for N > 1)."""

    def __init__(self, prob, local, rank, n_gpus, dist, comm="rccl"):
        import torch
        from slamgpu import ba
        self.prob, self.dist, self.local, self.rank, self.n = prob, dist, local, rank, n_gpus
        self.tdev = f"cuda:{local}" if comm == "rccl" else "cpu"   # gloo reduces host tensors
        self.solver = ba.BundleAdjuster(device=local)
        if n_gpus > 1 and comm == "host":
            def allreduce(arr, op):
                dist.all_reduce(torch.from_numpy(arr), op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM)
            self.solver.comm_init_host(n_gpus, rank, allreduce)
        elif n_gpus > 1:
            uid = ba.BundleAdjuster.unique_id() if rank == 0 else bytes(128)
            t = torch.tensor(list(uid), dtype=torch.uint8, device=f"cuda:{local}")
            dist.broadcast(t, 0)
            self.solver.comm_init(bytes(t.cpu().tolist()), n_gpus, rank)
        self.initial = prob.copy()
        self.solver.load(prob)

    def barrier(self):
        if self.dist is not None:
            self.dist.barrier()

    def max_over_ranks(self, x):
        if self.dist is None:
            return x
        import torch
        e = torch.tensor([x], dtype=torch.float64, device=self.tdev)
        self.dist.all_reduce(e, op=self.dist.ReduceOp.MAX)
        return float(e.item())

    def _timed_block(self, steps, warmup, always_lin):
        import torch
        from slamgpu.capi import default_solver_options
        g = self.solver
        g.begin(default_solver_options(max_num_iterations=warmup + 2 * steps + 16, disable_termination=1,
                                       always_linearize=always_lin))
        g.iterate(warmup)
        g.sync()
        s0 = g.summary()
        self.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.iterate(steps)
        g.sync()
        torch.cuda.synchronize()
        self.barrier()
        elapsed = self.max_over_ranks(time.perf_counter() - t0)
        s1 = g.summary()
        assert s1["sync_timeouts"] == 0 and s1["num_lm_iterations"] == warmup + steps, s1
        return elapsed, s0, s1

    def timed(self, steps, warmup, full=True, dump=False):
        """W warm-up then exactly K LM iterations (termination disabled, every iteration linearizes: the
        SURVEY.md 8d unit), barrier + synchronize on both sides, max over ranks; with `dump`, the state the
        K-th iteration left is then downloaded as a caller of the solver would receive it.  With `full`: then
        the same K with per-kernel HIP-event timing; then the same K in Ceres's regime (no linearization after
        a rejected step), reported beside the headline."""
        g = self.solver
        elapsed, s0, s1 = self._timed_block(steps, warmup, 1)
        outputs = None
        if dump:
            p = self.prob
            start = [a.copy() for a in (p.q, p.t, p.X, p.k)]
            g.download()   # into the arrays the solver was loaded from
            outputs = {"q": p.q.reshape(-1, 4).copy(), "t": p.t.reshape(-1, 3).copy(),
                       "X": p.X.reshape(-1, 4).copy(), "cost": np.array([s1["final_cost"]])}
            if p.cameras_free:
                outputs["k"] = p.k.reshape(-1, 7).copy()
            for a, b in zip((p.q, p.t, p.X, p.k), start):   # the later measurements start from the same problem
                a[:] = b
        head = {"elapsed": elapsed, "accepted": s1["num_successful_steps"] - s0["num_successful_steps"],
                "summary": s1, "outputs": outputs}
        if not full:
            return {**head, "kt": None, "work": None, "lin_active": None, "lm_regime": None}
        g.set_timing(True)
        g.iterate(steps)
        g.sync()
        kt = g.kernel_times()
        g.set_timing(False)
        s2 = g.summary()
        lm_elapsed, l0, l1 = self._timed_block(steps, warmup, 0)
        lm = {"ms_per_step": 1e3 * lm_elapsed / steps, "value": steps / lm_elapsed,
              "accepted_frac": (l1["num_successful_steps"] - l0["num_successful_steps"]) / steps,
              "note": "Ceres regime: a rejected step skips the linearization, so this figure depends on how many "
                      "of the K steps after W warm-up steps are rejected"}
        return {**head, "kt": kt, "work": g.kernel_work(),
                "lin_active": s2["num_lm_iterations"] - s1["num_lm_iterations"], "lm_regime": lm}

    def solve_from_start(self):
        """Complete solves from the perturbed start (termination on): iterations over wall time (includes
        the host's completion polls every 8 iterations and the result download), and the per-kernel
        device time per iteration from HIP events."""
        g = self.solver
        p = self.initial.copy()
        g.load(p)            # same structure: value-only reload of the perturbed start
        self.barrier()
        t0 = time.perf_counter()
        s = g.solve()
        wall = self.max_over_ranks(time.perf_counter() - t0)
        p = self.initial.copy()
        g.load(p)
        g.set_timing(True)
        g.solve()
        kt = g.kernel_times()
        g.set_timing(False)
        dev_ms = sum(v[0] * v[1] for v in kt.values())
        its = s["num_lm_iterations"]
        return {"lm_iterations": its, "accepted": s["num_successful_steps"], "termination": s["termination"],
                "final_cost": s["final_cost"], "wall_ms": 1e3 * wall, "iters_per_s_wall": its / wall if wall else None,
                "device_kernel_ms": dev_ms, "iters_per_s_device": its / (dev_ms * 1e-3) if dev_ms else None}


SPEC = os.environ.get("SG_SPEC", "1") != "0"   # speculative linearization (the library default)
KERNEL_SYMBOL = {"point_update": "k_update_lin" if SPEC else "k_point_update"}


def survey_fields(sb, ms, traffic):
    """The sweep priced on SURVEY 8d's algorithmic bytes (at the reference's f64: M 228 + P 148 + camera blocks)
    beside the implementation's own byte model (`frac`, which also counts the J records the chain re-reads and
    rewrites): achieved = those bytes over the same launch time, and the counter traffic as a multiple of them."""
    ach = sb / (ms * 1e-3) / 1e9
    return {"bytes_survey_model": sb, "achieved_survey_model": ach, "frac_survey_model": ach / HBM_PEAK_GBS,
            "traffic_over_survey_bytes": (traffic / sb) if traffic else None}


def kernel_report(res, steps, n_text, workload):
    """Per-iteration kernel times, the dominant kernel's roofline and the sweep roofline.  The Jacobian sweep of
    the timed iterations is k_update_lin (the candidate pass + the candidate's linearization) in the speculative
    chain, where k_linearize runs only in a solve's first iteration; k_linearize otherwise."""
    kt, work = res["kt"], res["work"]
    per_iter_ms = {k: v[0] * v[1] / max(steps, 1) for k, v in kt.items()}
    # the dominant kernel (the exchange timer of a multi-rank chain — pack, all-reduce, unpack — is not a kernel
    # and has no algorithmic work figure)
    dominant = max((k for k in per_iter_ms if k in work and k != "exchange"), key=per_iter_ms.get)
    dom_ms = kt[dominant][0]
    dom_bytes, dom_flops = work[dominant]
    if dom_flops > 0 and dominant == "cholesky":
        ach = dom_flops / (dom_ms * 1e-3) / 1e12
        roof = {"bound": "mfma", "achieved": ach, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": ach / FP64_PEAK_TFLOPS, **traffic_fields("k_chol_tiles", workload), "kernel": dominant,
                "us_per_launch": 1e3 * dom_ms,
                "note": "dissected tiled band Cholesky of the reduced camera system (two workgroups; %s), n^3/3 flops "
                        "over its mean HIP-event launch time" % n_text}
    else:
        ach = dom_bytes / (dom_ms * 1e-3) / 1e9
        sym = KERNEL_SYMBOL.get(dominant, "k_" + dominant)
        roof = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": ach / HBM_PEAK_GBS, **traffic_fields(sym, workload, dom_bytes), "kernel": sym,
                "us_per_launch": 1e3 * dom_ms}
        if dominant in ("linearize", "point_update") and "sweep_survey_model" in work:
            roof.update(survey_fields(work["sweep_survey_model"][0], dom_ms, roof.get("traffic")))
    if dominant == "schur" and dom_flops > 0:
        # k_schur runs its point elimination on the matrix cores: its v_mfma_f64_16x16x4f64 rate beside the HBM
        # price, and the matrix-core busy share the counters measured (VERDICT r4 Missing 3)
        achm = dom_flops / (dom_ms * 1e-3) / 1e12
        roof["mfma"] = {"achieved": achm, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achm / FP64_PEAK_TFLOPS,
                        "flops_per_launch_model": dom_flops,
                        **((pmc_mfma("k_schur", workload) or {}) if TRAFFIC_APPLIES else {}),
                        "note": "issued flops: 2048 per v_mfma_f64_16x16x4f64 (the window tiles a point touches, zero "
                                "tiles included) and 512 per v_mfma_f64_4x4x4_4b_f64 (its rhs slots), over the "
                                "HIP-event launch time"}
        useful = work.get("schur_useful", (0.0, 0.0))[1]
        if useful > 0:
            achu = useful / (dom_ms * 1e-3) / 1e12
            roof["mfma"].update({"useful_flops_per_launch": useful, "useful_achieved": achu,
                                 "useful_frac": achu / FP64_PEAK_TFLOPS,
                                 "useful_note": "the slots of each point's own tiles only (its first to its last "
                                                "window tile): the issued count less the zero tiles"})
    sweep = None
    n_lin = res["lin_active"]
    lk = "linearize" if kt.get("linearize", (0, 0))[1] > 0 else "point_update"
    if n_lin > 0 and kt.get(lk, (0, 0))[1] > 0:
        sym = "k_linearize" if lk == "linearize" else KERNEL_SYMBOL["point_update"]
        total_ms = kt[lk][0] * kt[lk][1]
        active = n_lin if lk == "linearize" else kt[lk][1]
        ach = work[lk][0] * active / (total_ms * 1e-3) / 1e9
        sweep = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                 "frac": ach / HBM_PEAK_GBS, "bytes_per_launch": work[lk][0], "kernel": sym,
                 **traffic_fields(sym, workload, work[lk][0]), "active_launches": active,
                 "launches": kt[lk][1]}
        if "sweep_survey_model" in work:
            sweep.update(survey_fields(work["sweep_survey_model"][0], total_ms / active, sweep.get("traffic")))
    return {k: round(v, 5) for k, v in per_iter_ms.items()}, roof, sweep


def run_workload(cfg, args, n_gpus, rank, local, dist, steps, warmup, weak=False, dump=False):
    full, prob, desc = make_workload(cfg, n_gpus, rank, args.points, args.frames, weak)
    r = Runner(prob, local, rank, n_gpus, dist, args.comm)
    res = r.timed(steps, warmup, args.full, dump)
    info = r.solver.info()
    start = r.solve_from_start() if args.full else None
    # shard balance: every rank's observations / pairs, gathered
    bal = None
    if dist is not None:
        import torch
        v = torch.tensor([prob.num_points, prob.num_obs, info["num_pairs"]], dtype=torch.float64,
                         device=r.tdev)
        allv = [torch.zeros_like(v) for _ in range(n_gpus)]
        dist.all_gather(allv, v)
        rows = [[int(x) for x in t.cpu().tolist()] for t in allv]
        bal = {"points": [x[0] for x in rows], "obs": [x[1] for x in rows], "schur_pairs": [x[2] for x in rows]}
        bal["pairs_max_over_mean"] = max(bal["schur_pairs"]) / (sum(bal["schur_pairs"]) / n_gpus)
    r.solver.close()
    return full, prob, desc, res, info, start, bal


def bench_sweep(local, sweep_obs):
    """Scaled sweep on a problem large enough to amortise launch latency: the linearization kernel alone
    (k_linearize, which the speculative chain runs once per solve), and the per-iteration sweep of that chain
    (k_update_lin: the point update, the candidate's linearization and its cost in one pass) timed inside K
    always-linearize LM iterations (`update_lin`)."""
    from slamgpu import ba
    from slamgpu.capi import default_solver_options
    from slamgpu.scene import make_scene
    npts = max(sweep_obs // 10, 1000)
    big = make_scene(num_frames=200, num_points=npts, seed=5, run_max=18)
    bp = ba.problem_from_map_frames(big, 198, 200, 2.0)
    bs = ba.BundleAdjuster(device=local)
    bs.load(bp)
    bs.begin(default_solver_options())
    bs.sweep(3)
    bs.sync()
    bs.set_timing(True)
    bs.sweep(20)
    bs.sync()
    kt = bs.kernel_times()["linearize"]
    wb = bs.kernel_work()["linearize"][0]
    sb = bs.kernel_work()["sweep_survey_model"][0]
    ach = wb / (kt[0] * 1e-3) / 1e9
    bs.close()
    # the per-iteration sweep: K LM iterations on the same problem, k_update_lin's HIP-event average
    bs = ba.BundleAdjuster(device=local)
    bs.load(bp.copy())
    bs.begin(default_solver_options(max_num_iterations=40, disable_termination=1, always_linearize=1))
    bs.iterate(3)
    bs.sync()
    bs.set_timing(True)
    bs.iterate(10)
    bs.sync()
    ku = bs.kernel_times()["point_update"]
    wu = bs.kernel_work()["point_update"][0]
    s1 = bs.summary()
    bs.close()
    assert s1["ok"] == 1 and s1["num_lm_iterations"] == 13, s1
    achu = wu / (ku[0] * 1e-3) / 1e9
    tl = traffic_fields("k_linearize", "sweep", wb)
    tu = traffic_fields("k_update_lin", "sweep", wu)
    return {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": ach / HBM_PEAK_GBS, "obs": bp.num_obs, "points": bp.num_points,
            "ms_per_launch": kt[0], "bytes_per_launch": wb, **tl, **survey_fields(sb, kt[0], tl.get("traffic")),
            "update_lin": {"kernel": "k_update_lin", "achieved": achu, "frac": achu / HBM_PEAK_GBS,
                           "ms_per_launch": ku[0], "bytes_per_launch": wu, "launches": ku[1],
                           **tu, **survey_fields(sb, ku[0], tu.get("traffic"))}}


def bench_solve_all(local, steps=20, warmup=3):
    """Whole-map refinements of main.cpp's calibration step (SolveAllFrames(map, 2, false / true), main.cpp:282,
    327; slam.cpp:447-480) on the config-2 map: every frame free but the gauge, and with solve_cameras the 7
    intrinsics of each camera couple every frame, so the reduced system is an arrowhead (the frame band bordered
    by 14 dense columns) and takes the bordered band solve (k_chol_tiles on the frames, k_chol_border for the
    intrinsics; SG_CHOL_BORDER=0: the one-workgroup k_cholesky_global).  LM iterations per second over K
    always-linearize iterations (termination off) and the per-kernel times."""
    from slamgpu import ba
    from slamgpu.capi import default_solver_options
    from slamgpu.scene import make_config
    m = make_config("C2")
    out = {}
    for cams in (False, True):
        p = ba.problem_from_map_all(m, 2.0, cams)
        g = ba.BundleAdjuster(device=local)
        g.load(p)
        info = g.info()
        g.begin(default_solver_options(max_num_iterations=warmup + 2 * steps + 8, disable_termination=1,
                                       always_linearize=1))
        g.iterate(warmup)
        g.sync()
        t0 = time.perf_counter()
        g.iterate(steps)
        g.sync()
        el = time.perf_counter() - t0
        s1 = g.summary()   # a solve that ended early would time no-op launches: refuse the figure
        assert s1["ok"] == 1 and s1["sync_timeouts"] == 0 and s1["num_lm_iterations"] == warmup + steps, s1
        g.set_timing(True)
        g.iterate(steps)
        g.sync()
        kt = g.kernel_times()
        s2 = g.summary()
        assert s2["ok"] == 1 and s2["sync_timeouts"] == 0 and s2["num_lm_iterations"] == warmup + 2 * steps, s2
        g.close()
        out["solve_cameras" if cams else "poses_points"] = {
            "iters_per_s": steps / el, "ms_per_iter": 1e3 * el / steps, "n": info["n"],
            "cholesky": info["cholesky"], "band_tiles": info["band_tiles"],
            "kernel_ms_per_iter": {k: round(v[0] * v[1] / steps, 5) for k, v in kt.items()}}
    return out


REPLICATED = ("cam_finalize", "cholesky", "decide")   # every landmark shard runs these on the whole system


def model_scaling(local, full, full_kernel_ms, ns=(2, 4, 8), steps=20, warmup=3, allreduce_us=20.0, band_gbs=50.0,
                  decide_us=0.0):
    """Modelled strong scaling of a BA workload over N landmark shards, from measured kernel times.  Every shard of
    the N-way split (sg_problem_shard) is loaded alone on this GPU and timed with the multi-rank chain forced
    (SG_XCHG_MERGE=force: each rank assembles its own camera blocks into its partial S, the band of S travels
    packed with the camera gradient / diagonal / cost scalars in its tail, and the bookkeeping and damping follow
    the exchange; the pack and unpack kernels are timed as 'exchange').  A shard's iteration = its shardable
    kernels (linearize, camera reduce, Schur, S reduce, point update + next linearization, update reduce, pack /
    unpack) + the replicated ones measured on the whole problem in the same chain (camera finalize, Cholesky, the
    decision launch k_decide, timed in the forced merged chain) + `decide_us` of any further unmeasured launch +
    two all-reduces per iteration (the
    packed band with its tail, the step scalars) priced at `allreduce_us` each plus the band at `band_gbs`
    (assumptions, not measurements: RCCL over xGMI is not measurable on this 1-GPU box).  The slowest shard sets
    the pace."""
    from slamgpu import ba
    from slamgpu.capi import default_solver_options

    def per_iter(prob):
        g = ba.BundleAdjuster(device=local)
        g.load(prob)
        info = g.info()
        g.begin(default_solver_options(max_num_iterations=warmup + steps + 4, disable_termination=1,
                                       always_linearize=1))
        g.iterate(warmup)
        g.sync()
        g.set_timing(True)
        g.iterate(steps)
        g.sync()
        kt = g.kernel_times()
        g.close()
        return {k: v[0] * v[1] / steps for k, v in kt.items()}, info

    old = os.environ.get("SG_XCHG_MERGE")
    os.environ["SG_XCHG_MERGE"] = "force"
    try:
        full_ms, info = per_iter(full)
        rep_ms = sum(full_ms.get(k, 0.0) for k in REPLICATED) + decide_us * 1e-3
        band = 8.0 * info["n"] * min(info["n"], 16 * (info["band_tiles"] + 1)) + 8.0 * 2 * info["n"]
        one_ms = sum(full_kernel_ms.values())
        out = {"n": [1], "ms_per_iter": [one_ms], "speedup": [1.0], "replicated_ms": rep_ms,
               "replicated_kernels_ms": {k: full_ms.get(k, 0.0) for k in REPLICATED},
               "shard_compute_ms": [one_ms - sum(full_kernel_ms.get(k, 0.0) for k in REPLICATED)],
               "allreduce_ms": [0.0], "exchanges_per_iteration": 2}
        for n in ns:
            worst = 0.0
            for r in range(n):
                ms, _ = per_iter(ba.shard_problem(full, r, n))
                worst = max(worst, sum(v for k, v in ms.items() if k not in REPLICATED))
            ar_ms = 2 * allreduce_us * 1e-3 + band / (band_gbs * 1e9) * 1e3
            t = worst + rep_ms + ar_ms
            out["n"].append(n)
            out["shard_compute_ms"].append(worst)
            out["allreduce_ms"].append(ar_ms)
            out["ms_per_iter"].append(t)
            out["speedup"].append(one_ms / t)
    finally:
        if old is None:
            del os.environ["SG_XCHG_MERGE"]
        else:
            os.environ["SG_XCHG_MERGE"] = old
    out["assumptions"] = ("2 all-reduces per iteration at %.0f us each + the packed band and tail at %.0f GB/s, a "
                          "separate decision launch of %.0f us; the slowest shard's measured shardable kernels "
                          "(multi-rank chain forced on one rank) + the whole problem's replicated kernels (%s)"
                          % (allreduce_us, band_gbs, decide_us, ", ".join(REPLICATED)))
    return out


DUMP_BUDGET = 64e6   # bytes of --dump-outputs files in all


def write_outputs(out_dir, outputs, rank, n_gpus):
    """--dump-outputs: every array as out_dir/<name>.npy (float64; a rank of N > 1 writes its own shard as
    <name>_rank<r>.npy).  Arrays are written whole while they fit DUMP_BUDGET together; beyond it, each array
    over its share is cut to a fixed seeded sample of its rows (in row order)."""
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BUDGET / n_gpus / max(len(outputs), 1)
    whole = sum(a.nbytes for a in outputs.values()) * n_gpus <= DUMP_BUDGET
    for name, a in outputs.items():
        a = np.ascontiguousarray(a, dtype=np.float64)
        if not whole and a.nbytes > share:
            keep = max(1, int(share // (a.nbytes // len(a))))
            a = a[np.sort(np.random.default_rng(0).choice(len(a), keep, replace=False))]
        np.save(os.path.join(out_dir, name + ("_rank%d" % rank if n_gpus > 1 else "") + ".npy"), a)


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n):
    """`--gpus N` (N > 1) with no launcher in the environment: start the N rank processes under
    torch.distributed.run as CHILDREN of this process (nothing here has touched the GPU: no HIP call, no
    torch.cuda query), with this command line, so rank 0's JSON line reaches stdout exactly as in the driver's
    own torchrun form.  Returns the launcher's exit status (non-zero if any rank failed)."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def check_world(args, ws):
    """The rank count must be the one asked for: a launcher's WORLD_SIZE equal to --gpus, and with RCCL one GPU per
    rank.  A mismatch exits non-zero instead of printing a line for the wrong N."""
    if ws != args.gpus:
        sys.exit("bench.py: WORLD_SIZE=%d but --gpus %d: refusing to report a line for the wrong rank count"
                 % (ws, args.gpus))
    if ws > 1 and args.comm == "rccl":
        import torch
        if torch.cuda.device_count() < ws:
            sys.exit("bench.py: --gpus %d --comm rccl needs one GPU per rank, %d visible (use --comm host to "
                     "rehearse several ranks on one GPU)" % (ws, torch.cuda.device_count()))


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    ws, rank, local = dist_env()
    check_world(args, ws)
    import torch

    if args.only in ("sweep", "frontend"):   # profiling runs of one non-headline workload (N = 1)
        out = bench_sweep(local, args.sweep_obs) if args.only == "sweep" else \
            {"tracker": bench_tracker(local, 0), "hamming": bench_hamming(local, 0)}
        print(json.dumps({"only": args.only, "result": out}), flush=True)
        return

    if args.comm == "host":   # rehearsal: several ranks may share the box's GPUs
        local = local % max(1, torch.cuda.device_count())
    dist = None
    if ws > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        dist.init_process_group("nccl" if args.comm == "rccl" else "gloo", rank=rank, world_size=ws)
    n_gpus = ws
    c5 = args.config == "C5"
    global TRAFFIC_APPLIES
    TRAFFIC_APPLIES = n_gpus == 1

    full, prob, desc, res, info, start, bal = run_workload(args.config, args, n_gpus, rank, local, dist,
                                                           args.steps, args.warmup,
                                                           dump=args.dump_outputs is not None)
    if args.dump_outputs is not None:
        write_outputs(args.dump_outputs, res["outputs"], rank, n_gpus)
    other = None
    if args.other:
        ocfg = "C2" if c5 else "C5"
        k2 = min(args.steps, 50)
        f2, p2, d2, r2, i2, st2, b2 = run_workload(ocfg, args, n_gpus, rank, local, dist, k2, min(args.warmup, 10))
        if rank == 0:
            pk2, roof2, sw2 = kernel_report(r2, k2, "n=%d, band %d tiles" % (i2["n"], i2["band_tiles"]), ocfg)
            val2 = k2 / r2["elapsed"]
            scal = None
            if n_gpus == 1 and args.model_scaling:
                scal = model_scaling(local, f2, pk2)
            other = {"workload": d2, "scaling": "strong", "value": val2,
                     "unit": "iters/s", "steps": k2, "ms_per_step": 1e3 * r2["elapsed"] / k2,
                     "accepted_frac": r2["accepted"] / k2, "lm_regime": r2["lm_regime"], "keyframes": f2.num_frames,
                     "landmarks": f2.num_points, "observations": f2.num_obs, "per_rank": {
                         "landmarks": p2.num_points, "observations": p2.num_obs}, "solver": i2,
                     "kernel_ms_per_iter": pk2, "roofline": roof2, "roofline_sweep": sw2,
                     "solve_from_start": st2, "shard_balance": b2, "strong_scaling_model": scal}

    weak = None
    if n_gpus > 1 and args.weak and not c5:
        # C2 weak scaling beside the strong headline: 50 keyframes and N x 20k landmarks, N x K / time
        kw = min(args.steps, 50)
        fw, pw, dw, rw, iw, stw, bw = run_workload("C2", args, n_gpus, rank, local, dist, kw, min(args.warmup, 10),
                                                   weak=True)
        weak = {"workload": dw, "scaling": "weak", "value": n_gpus * kw / rw["elapsed"],
                "unit": "iters/s (config-2 iterations: N x K / time)", "steps": kw,
                "ms_per_step": 1e3 * rw["elapsed"] / kw, "landmarks": fw.num_points, "observations": fw.num_obs,
                "per_rank": {"landmarks": pw.num_points, "observations": pw.num_obs}, "shard_balance": bw}

    if rank != 0:
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return

    per_iter_ms, roof, sweep = kernel_report(res, args.steps, "n=%d, band %d tiles" % (info["n"], info["band_tiles"]),
                                             args.config) if args.full else (None, None, None)
    scal1 = model_scaling(local, full, per_iter_ms) if n_gpus == 1 and args.model_scaling else None

    sweep_scaled = bench_sweep(local, args.sweep_obs) if args.sweep_obs > 0 and n_gpus == 1 else None
    solve_all = bench_solve_all(local) if args.solve_all and n_gpus == 1 else None

    cpu = None
    if args.cpu_runs > 0 and n_gpus == 1:
        cpu = cpu_legs(full, args.cpu_runs, "48, 50, 2.0" if not c5 else "198, 200, 2.0")

    frontend = None
    if args.frontend and n_gpus == 1:
        cs = args.cpu_seconds
        frontend = {"tracker": bench_tracker(local, cs), "hamming": bench_hamming(local, cs),
                    "matcher": bench_matcher_sequence(local, cs > 0)}

    value = args.steps / res["elapsed"]
    line = {
        "metric": "local-BA iters/sec (%s)" % ("200 KF, 200k pts" if c5 else "50 KF, 20k pts"),
        "value": value,
        "unit": "iters/s",
        "n_gpus": n_gpus,
        "ranks": {"world_size": ws, "solver_nranks": info["nranks"], "num_allreduces": info["num_allreduces"],
                  "comm": args.comm if n_gpus > 1 else None},
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * res["elapsed"] / args.steps,
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic (seeded scene generator, slamgpu/scene.py)",
        "config": {"workload": desc, "keyframes": full.num_frames, "landmarks": full.num_points,
                   "observations": full.num_obs, "landmarks_per_gpu": prob.num_points,
                   "observations_per_gpu": prob.num_obs, "free_frames": int(full.frame_rot_free.sum()),
                   "parallelism": ("landmark-shard x%d (RCCL all-reduce of the camera system)" % n_gpus
                                   if args.comm == "rccl" else
                                   "landmark-shard x%d ranks over a host transport (gloo; rehearsal, not a "
                                   "multi-GPU measurement)" % n_gpus) if n_gpus > 1 else "single GPU"},
        "accepted_frac": res["accepted"] / args.steps,
        "timed_regime": "every LM iteration linearizes (sg_solver_options.always_linearize; SURVEY.md 8d unit)",
        "lm_regime": res["lm_regime"],
        "solve_from_start": start,
        "solver": info,
        "roofline": roof,
        "roofline_sweep": sweep,
        "roofline_sweep_scaled": sweep_scaled,
        "solve_all_frames": solve_all,
        "kernel_ms_per_iter": per_iter_ms,
        "cpu_baseline": cpu,
        "speedup_vs_cpu": (value / cpu["value"]) if cpu and cpu["value"] else None,
        "speedup_vs_cpu_from_start": (start["iters_per_s_wall"] / cpu["value"])
        if cpu and cpu["value"] and start and start["iters_per_s_wall"] else None,
        "lm_state": {"final_cost": res["summary"]["final_cost"], "radius": res["summary"]["trust_region_radius"]},
        "shard_balance": bal,
        "strong_scaling_model": scal1,
        "weak_scaling": weak,
        "other_workload": other,
        "frontend": frontend,
        "traffic_source": "HBM bytes per launch from rocprofv3 --pmc FETCH_SIZE/WRITE_SIZE passes over "
                          "bench.py --only <workload> --steps 20 --warmup 5 (tools/profile_round.sh, "
                          "profiles/*_pmc_traffic_<workload>.json; FETCH_SIZE doubled on gfx950)",
    }
    print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
