"""Python mirror of the reference's Slam interface (slam.h:21-65) over libslamgpu.so.

`Slam` keeps the reference's method names and semantics (SolveFrames / SolveAllFrames / ReprojectMap,
iterations(), error()); `BundleAdjuster` exposes the device solver directly for benchmarks and the
landmark-sharded multi-GPU path.  All compute runs in the HIP library; these classes only marshal.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import (ProblemArrays, SgBaInfo, SgDeviceOptions, SgLocalizeOptions, SgLocalizeResult, SgProblem,
                   SgSolverOptions, SgSolverSummary, SgTriangulateOptions, SgTriangulateResult, check,
                   default_solver_options, load_library)
from .scene import MapArrays


def _dev(device=0, precision=0, rank=0, nranks=1):
    return SgDeviceOptions(device=device, precision=precision, rank=rank, nranks=nranks)


def _epipolar_side(keypoints, n):
    """One side's per-pair (pixels, descriptors[, levels]) tuples -> offsets, flat pixels, descriptors, levels."""
    if len(keypoints) != n:
        raise ValueError("one (pixels, descriptors[, levels]) tuple per listed pair")
    xys = [np.ascontiguousarray(k[0], dtype=np.float64).reshape(-1, 2) for k in keypoints]
    dss = [np.ascontiguousarray(k[1], dtype=np.uint64).reshape(-1, 4) for k in keypoints]
    if any(len(a) != len(b) for a, b in zip(xys, dss)):
        raise ValueError("one descriptor per keypoint")
    with_levels = [len(k) > 2 and k[2] is not None for k in keypoints]
    if n and any(with_levels) != all(with_levels):
        raise ValueError("levels for every pair or for none")
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(a) for a in xys])
    K = int(off[n])
    xy = np.concatenate(xys).reshape(-1) if K else np.zeros(0)
    ds = np.concatenate(dss).reshape(-1) if K else np.zeros(0, dtype=np.uint64)
    lv = None
    if n and all(with_levels):
        lvs = [np.ascontiguousarray(k[2], dtype=np.int32).reshape(-1) for k in keypoints]
        if any(len(a) != len(b) for a, b in zip(xys, lvs)):
            raise ValueError("one level per keypoint")
        lv = np.concatenate(lvs) if K else np.zeros(0, dtype=np.int32)
    return off, xy, ds, lv


def _match_epipolar(fn, m, pairs, keypoints_a, keypoints_b, tol_px, min_parallax, max_dist, ratio_percent, what):
    """Marshal one sg_slam_match_epipolar-shaped call (fn takes the arguments after the handle) and return one
    result dict per listed pair."""
    from .capi import SgEpipolarOptions, SgEpipolarResult
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    n = len(pr)
    ao, axy, ads, alv = _epipolar_side(keypoints_a, n)
    bo, bxy, bds, blv = _epipolar_side(keypoints_b, n)
    if (alv is None) != (blv is None):
        raise ValueError("levels on both sides or on neither")
    KA = int(ao[n])
    out = [np.full(max(KA, 1), 7, dtype=np.int32) for _ in range(5)]
    res = (SgEpipolarResult * max(n, 1))()
    opt = SgEpipolarOptions(tol_px=tol_px, min_parallax=min_parallax, max_dist=max_dist, ratio_percent=ratio_percent)
    ms = m.struct()
    ip, dp, up = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    lvl = lambda a: None if a is None else a.ctypes.data_as(ip)   # noqa: E731
    # (empty arrays are passed by address: only the counts decide whether they are read)
    check(fn(C.byref(ms), pr.ctypes.data_as(ip), n, ao.ctypes.data_as(ip), axy.ctypes.data_as(dp),
             ads.ctypes.data_as(up), lvl(alv), bo.ctypes.data_as(ip), bxy.ctypes.data_as(dp), bds.ctypes.data_as(up),
             lvl(blv), C.byref(opt), *[a.ctypes.data_as(ip) for a in out], res), what)
    names = ("match", "best_kp", "best_dist", "second_dist", "num_candidates")
    results = []
    for i in range(n):
        d = res[i].as_dict()
        for name, a in zip(names, out):
            d[name] = a[ao[i]:ao[i + 1]].copy()
        results.append(d)
    return results


def match_epipolar_cpu(m: MapArrays, pairs, keypoints_a, keypoints_b, tol_px: float = 2.0, min_parallax: float = 0.0,
                       max_dist: int = 64, ratio_percent: int = 80) -> list:
    """Slam.MatchEpipolar answered by the planner's CPU executor on the calling thread (a diagnostic entry point of
    the library: no handle, no device).  Returns what Slam.epipolar_match_results() returns."""
    from .capi import SgEpipolarOptions, SgEpipolarResult, SgMap
    fn = load_library().sg_debug_match_epipolar_cpu
    ip, dp, up = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(SgMap), ip, C.c_int32, ip, dp, up, ip, ip, dp, up, ip, C.POINTER(SgEpipolarOptions), ip, ip,
                   ip, ip, ip, C.POINTER(SgEpipolarResult)]
    return _match_epipolar(fn, m, pairs, keypoints_a, keypoints_b, tol_px, min_parallax, max_dist, ratio_percent,
                           "match_epipolar_cpu")


def problem_from_map_frames(m: MapArrays, num_to_solve: int, num_to_present: int, range_: float = 2.0):
    """Slam::SolveFrames selection + SetupProblem (slam.cpp:257-443) -> ProblemArrays, or None on abort."""
    lib = load_library()
    p = SgProblem()
    built = C.c_int32()
    ms = m.struct()
    check(lib.sg_problem_from_map_frames(C.byref(ms), num_to_solve, num_to_present, range_, C.byref(p),
                                         C.byref(built)), "sg_problem_from_map_frames")
    if not built.value:
        return None
    pa = ProblemArrays.from_struct(p)
    lib.sg_problem_free(C.byref(p))
    return pa


def problem_from_map_all(m: MapArrays, range_: float = 2.0, solve_cameras: bool = False):
    lib = load_library()
    p = SgProblem()
    built = C.c_int32()
    ms = m.struct()
    check(lib.sg_problem_from_map_all(C.byref(ms), range_, int(solve_cameras), C.byref(p), C.byref(built)),
          "sg_problem_from_map_all")
    if not built.value:
        return None
    pa = ProblemArrays.from_struct(p)
    lib.sg_problem_free(C.byref(p))
    return pa


def shard_problem(pa: ProblemArrays, rank: int, nranks: int) -> ProblemArrays:
    """Landmark shard `rank` of `nranks` (points split by first observing frame; frames replicated)."""
    lib = load_library()
    out = SgProblem()
    ps = pa.struct()
    check(lib.sg_problem_shard(C.byref(ps), rank, nranks, C.byref(out)), "sg_problem_shard")
    sh = ProblemArrays.from_struct(out)
    lib.sg_problem_free(C.byref(out))
    return sh


class LocalCommGroup:
    """sg_comm_group: nranks solver handles on one device exchanging in-process instead of over RCCL."""

    def __init__(self, nranks: int):
        self.lib = load_library()
        self.h = C.c_void_p()
        check(self.lib.sg_comm_group_create(C.byref(self.h), nranks), "sg_comm_group_create")

    def close(self):
        if self.h:
            self.lib.sg_comm_group_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BundleAdjuster:
    """The device solver (sg_ba): load a problem, solve or run fixed LM iterations."""

    def __init__(self, device: int = 0, precision: int = 0):
        self.lib = load_library()
        self.h = C.c_void_p()
        dev = _dev(device, precision)
        check(self.lib.sg_ba_create(C.byref(self.h), C.byref(dev)), "sg_ba_create")
        self._pa = None

    def close(self):
        if self.h:
            self.lib.sg_ba_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def comm_init(self, uid: bytes, nranks: int, rank: int):
        buf = C.create_string_buffer(uid, 128)
        check(self.lib.sg_ba_comm_init(self.h, buf, nranks, rank), "sg_ba_comm_init")

    def comm_init_local(self, group: "LocalCommGroup", rank: int):
        """Join an in-process communicator group (one device, one host thread per rank; tests)."""
        check(self.lib.sg_ba_comm_init_local(self.h, group.h, rank), "sg_ba_comm_init_local")

    def comm_init_host(self, nranks: int, rank: int, allreduce):
        """Join a host-transport communicator (sg_ba_comm_init_host): allreduce(array, op) receives each of the
        solver's all-reduce buffers as a float64 numpy view of pinned host memory (op "sum" or "max") and
        reduces it in place across the ranks (e.g. torch.distributed over gloo, one process per rank)."""
        import numpy as np
        from .capi import ALLREDUCE_FN

        def cb(buf, n, op, user):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(int(n),)), "max" if op == 1 else "sum")
                return 0
            except Exception:   # noqa: BLE001 - reported to the solver as SG_ECOMM
                return 1
        self._allreduce_cb = ALLREDUCE_FN(cb)   # kept alive as long as the handle
        check(self.lib.sg_ba_comm_init_host(self.h, nranks, rank, C.cast(self._allreduce_cb, C.c_void_p), None),
              "sg_ba_comm_init_host")

    @staticmethod
    def unique_id() -> bytes:
        lib = load_library()
        buf = C.create_string_buffer(128)
        check(lib.sg_comm_unique_id(buf), "sg_comm_unique_id")
        return buf.raw

    def load(self, pa: ProblemArrays):
        self._pa = pa
        ps = pa.struct()
        check(self.lib.sg_ba_load(self.h, C.byref(ps)), "sg_ba_load")

    def reserve(self, max_frames: int, max_points: int, max_obs: int):
        """Pre-size the device / pinned buffers for problems up to this size (drops the loaded problem if it
        reallocates)."""
        check(self.lib.sg_ba_reserve(self.h, max_frames, max_points, max_obs), "sg_ba_reserve")

    def load_counts(self) -> tuple:
        """(full loads, value-only loads): a load with the previous load's structure reuses its index lists."""
        full, vals = C.c_int32(0), C.c_int32(0)
        check(self.lib.sg_ba_load_counts(self.h, C.byref(full), C.byref(vals)), "sg_ba_load_counts")
        return full.value, vals.value

    def info(self) -> dict:
        """What the last load set up: sizes, Cholesky band and path, Schur pair count, shard."""
        i = SgBaInfo()
        check(self.lib.sg_ba_info_get(self.h, C.byref(i)), "sg_ba_info_get")
        return i.as_dict()

    def solve(self, options: SgSolverOptions = None) -> dict:
        o = options or default_solver_options()
        s = SgSolverSummary()
        ps = self._pa.struct()
        check(self.lib.sg_ba_solve(self.h, C.byref(o), C.byref(ps), C.byref(s)), "sg_ba_solve")
        return s.as_dict()

    def begin(self, options: SgSolverOptions):
        check(self.lib.sg_ba_begin(self.h, C.byref(options)), "sg_ba_begin")

    def iterate(self, n: int):
        check(self.lib.sg_ba_iterate(self.h, n), "sg_ba_iterate")

    def sweep(self, n: int):
        """n Jacobian/Hessian sweeps (k_linearize) at the current state — benchmark of the HBM kernel."""
        check(self.lib.sg_ba_sweep(self.h, n), "sg_ba_sweep")

    def sync(self):
        check(self.lib.sg_ba_sync(self.h), "sg_ba_sync")

    def summary(self) -> dict:
        s = SgSolverSummary()
        check(self.lib.sg_ba_summary(self.h, C.byref(s)), "sg_ba_summary")
        return s.as_dict()

    def download(self):
        ps = self._pa.struct()
        check(self.lib.sg_ba_download(self.h, C.byref(ps)), "sg_ba_download")

    def evaluate(self):
        n = self._pa.num_obs
        r = np.zeros(2 * n)
        cost = C.c_double()
        nf = C.c_int32()
        check(self.lib.sg_ba_evaluate(self.h, r.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cost),
                                      C.byref(nf)), "sg_ba_evaluate")
        return r.reshape(-1, 2), cost.value, nf.value

    def set_timing(self, on: bool):
        check(self.lib.sg_ba_set_timing(self.h, int(on)), "sg_ba_set_timing")

    def kernel_times(self) -> dict:
        names = C.create_string_buffer(1024)
        ms = np.zeros(32)
        cnt = np.zeros(32, dtype=np.int32)
        check(self.lib.sg_ba_kernel_times(self.h, names, 1024, ms.ctypes.data_as(C.POINTER(C.c_double)),
                                          cnt.ctypes.data_as(C.POINTER(C.c_int32)), 32), "sg_ba_kernel_times")
        nm = names.value.decode().split(",")
        return {n: (float(ms[i]), int(cnt[i])) for i, n in enumerate(nm)}

    def kernel_work(self) -> dict:
        by = np.zeros(32)
        fl = np.zeros(32)
        check(self.lib.sg_ba_kernel_work(self.h, by.ctypes.data_as(C.POINTER(C.c_double)),
                                         fl.ctypes.data_as(C.POINTER(C.c_double)), 32), "sg_ba_kernel_work")
        names = ["linearize", "cam_reduce", "cam_finalize", "schur", "S_reduce", "cholesky", "point_update",
                 "upd_reduce", "decide"]
        out = {n: (float(by[i]), float(fl[i])) for i, n in enumerate(names)}
        # derived figures after the kernels' slots (KernelWork, ba_solver.hip): k_schur's useful flops (no zero
        # tiles) and SURVEY 8d's algorithmic bytes of one linearization sweep at f64
        out["schur_useful"] = (0.0, float(fl[10]))
        out["sweep_survey_model"] = (float(by[11]), 0.0)
        return out


class Slam:
    """slam.h:21-65 — the reference's Slam object, backed by the MI355X solver."""

    def __init__(self, device: int = 0, options: SgSolverOptions = None):
        self.lib = load_library()
        self.h = C.c_void_p()
        dev = _dev(device)
        check(self.lib.sg_slam_create(C.byref(self.h), C.byref(dev)), "sg_slam_create")
        if options is not None:
            check(self.lib.sg_slam_set_options(self.h, C.byref(options)), "sg_slam_set_options")

    def __del__(self):
        try:
            if self.h:
                self.lib.sg_slam_destroy(self.h)
        except Exception:
            pass

    def SolveFrames(self, m: MapArrays, num_to_solve: int, num_to_present: int, range_: float) -> bool:
        solved = C.c_int32()
        ms = m.struct()
        check(self.lib.sg_slam_solve_frames(self.h, C.byref(ms), num_to_solve, num_to_present, range_,
                                            C.byref(solved)), "Slam::SolveFrames")
        return bool(solved.value)

    def SolveAllFrames(self, m: MapArrays, range_: float, solve_cameras: bool) -> bool:
        solved = C.c_int32()
        ms = m.struct()
        check(self.lib.sg_slam_solve_all_frames(self.h, C.byref(ms), range_, int(solve_cameras),
                                                C.byref(solved)), "Slam::SolveAllFrames")
        return bool(solved.value)

    def SolveFramePose(self, f1, f2) -> bool:
        """slam.cpp:180-182: the reference returns false unconditionally (dead code after the return)."""
        return False

    def SolveFramePoses(self, m: MapArrays, frames, range_: float, with_frame_distance: bool = False) -> list:
        """Pose-only bundle adjustment (sg_slam_solve_frame_poses): each listed frame's pose against the map's
        points as they are, all frames in one device launch.  Updates m.q / m.t of the solved frames in place and
        returns one bool per listed frame; frame_pose_summaries() has their summaries."""
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        n = len(fr)
        solved = np.zeros(n, dtype=np.int32)
        sums = (SgSolverSummary * max(n, 1))()
        ms = m.struct()
        check(self.lib.sg_slam_solve_frame_poses(self.h, C.byref(ms), fr.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                                 range_, int(with_frame_distance),
                                                 solved.ctypes.data_as(C.POINTER(C.c_int32)), sums),
              "Slam::SolveFramePoses")
        self._pose_summaries = [sums[i].as_dict() for i in range(n)]
        return [bool(v) for v in solved]

    def frame_pose_summaries(self) -> list:
        """Summary dicts of the last SolveFramePoses call, or of the polish of the last LocalizeFrames call, one per
        listed frame."""
        return list(getattr(self, "_pose_summaries", []))

    def LocalizeFrames(self, m: MapArrays, frames, threshold_px: float = 4.0, max_hypotheses: int = 1024,
                       min_inliers: int = 8, seed: int = 0, refine: bool = True, range_: float = 2.0) -> list:
        """Localization from scratch (sg_slam_localize_frames): each listed frame's pose from its usable
        observations and the map's points as they are, by P3P RANSAC on the device (max_hypotheses three-point
        samples per frame, MSAC at threshold_px) and, with refine, SolveFramePoses' solver (CauchyLoss(range_)) from
        the winner.  The pose at entry is not read.  Updates m.q / m.t of the localized frames in place and returns
        one bool per listed frame; localization_results() has their statuses and figures,
        localization_inliers() the per-observation inlier flags, frame_pose_summaries() the polish's summaries."""
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        n = len(fr)
        solved = np.zeros(n, dtype=np.int32)
        res = (SgLocalizeResult * max(n, 1))()
        sums = (SgSolverSummary * max(n, 1))()
        inl = np.full(max(m.num_obs, 1), -1, dtype=np.int32)
        opt = SgLocalizeOptions(threshold_px=threshold_px, max_hypotheses=max_hypotheses, min_inliers=min_inliers,
                                seed=seed, refine=int(bool(refine)), range=range_)
        ms = m.struct()
        check(self.lib.sg_slam_localize_frames(self.h, C.byref(ms), fr.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                               C.byref(opt), solved.ctypes.data_as(C.POINTER(C.c_int32)), res,
                                               inl.ctypes.data_as(C.POINTER(C.c_int32)), sums),
              "Slam::LocalizeFrames")
        self._localization_results = [res[i].as_dict() for i in range(n)]
        self._localization_inliers = inl[:m.num_obs]
        self._pose_summaries = [sums[i].as_dict() for i in range(n)]
        return [bool(v) for v in solved]

    def localization_results(self) -> list:
        """Result dicts of the last LocalizeFrames call, one per listed frame: status (a LOC_STATUS name), num_obs,
        num_inliers, refined, best_hypothesis, best_sample, hypotheses, models, msac_cost, inlier_rms_px,
        ransac_cost and the RANSAC winner's q, t (before the polish)."""
        return list(getattr(self, "_localization_results", []))

    def localization_inliers(self) -> np.ndarray:
        """int32 per observation of the map after the last LocalizeFrames call: 1 / 0 for the records of the
        localized frames at the written pose, -1 everywhere else."""
        return np.array(getattr(self, "_localization_inliers", np.zeros(0, dtype=np.int32)))

    def RelativePoses(self, m: MapArrays, pairs, threshold_px: float = 2.0, max_hypotheses: int = 1024,
                      min_inliers: int = 16, min_parallax: float = 0.0, seed: int = 0, refine: bool = True,
                      baseline: float = 0.0) -> list:
        """Relative pose of frame pairs (sg_slam_relative_poses): for each listed pair (a, b), where b is relative to
        a, from the pixels of the points both observe alone, by 8-point RANSAC on the device (max_hypotheses
        eight-record samples per pair, MSAC on the Sampson distance at threshold_px, local optimisation with refine).
        Neither pose and no point is read.  With baseline > 0, frame b of each solved pair is written into m.q / m.t
        at that distance from a's pose as it was at entry; with 0 the map is left alone.  Returns one bool per pair;
        relative_pose_results() has the statuses, q_rel, the unit t_rel and E, relative_pose_records() the per-record
        inlier mask and observation indices."""
        from .capi import SgRelposeOptions, SgRelposeResult
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        n = len(pr)
        solved = np.zeros(n, dtype=np.int32)
        res = (SgRelposeResult * max(n, 1))()
        in_range = (pr[:, 0] >= 0) & (pr[:, 0] < m.num_frames)
        cap = int(np.bincount(m.obs_frame, minlength=max(m.num_frames, 1))[pr[in_range, 0]].sum()) if n else 0
        off = np.zeros(n + 1, dtype=np.int32)
        inl = np.full(max(cap, 1), -1, dtype=np.int32)
        obs = np.full(2 * max(cap, 1), -1, dtype=np.int32)
        opt = SgRelposeOptions(threshold_px=threshold_px, max_hypotheses=max_hypotheses, min_inliers=min_inliers,
                               min_parallax=min_parallax, seed=seed, refine=int(bool(refine)), baseline=baseline)
        ms = m.struct()
        ip = C.POINTER(C.c_int32)
        check(self.lib.sg_slam_relative_poses(self.h, C.byref(ms), pr.ctypes.data_as(ip), n, C.byref(opt),
                                              solved.ctypes.data_as(ip), res, off.ctypes.data_as(ip),
                                              inl.ctypes.data_as(ip), obs.ctypes.data_as(ip), cap),
              "Slam::RelativePoses")
        self._relpose_results = [res[i].as_dict() for i in range(n)]
        total = int(off[n])
        self._relpose_records = (off, inl[:total].copy(), obs[:2 * total].reshape(-1, 2).copy())
        return [bool(v) for v in solved]

    def relative_pose_results(self) -> list:
        """Result dicts of the last RelativePoses call, one per pair: status (a REL_STATUS name), num_obs,
        num_inliers, num_front, num_parallax, refined, best_hypothesis, best_sample, hypotheses, models, msac_cost,
        ransac_cost, inlier_rms_px, q, t and E (3 x 3)."""
        return list(getattr(self, "_relpose_results", []))

    def relative_pose_records(self) -> tuple:
        """(offsets [n + 1], inlier mask per record: 1 / 0 for solved pairs and -1 elsewhere, observation indices
        per record: in a, in b) of the last RelativePoses call."""
        return getattr(self, "_relpose_records", (np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32),
                                                  np.zeros((0, 2), dtype=np.int32)))

    def AlignPoints(self, m: MapArrays, groups, threshold: float = 10.0, max_hypotheses: int = 1024,
                    min_inliers: int = 8, seed: int = 0, refine: bool = True, fix_scale: bool = False,
                    max_scale: float = 0.0, min_gap: float = 1e-6) -> list:
        """Alignment of matched landmarks (sg_slam_align_points): for each group, a (K, 2) array of map point indices
        (point a, point b), the similarity Y = scale R(q) X + t that takes the a side onto the b side, by 3-point
        Sim(3) RANSAC on the device (max_hypotheses samples per group, MSAC on the distance in b's coordinates at
        threshold, local optimisation with refine).  The map is not written: ApplySimilarity does that.  Returns one
        result dict per group: the fields of sg_align_result with status as an ALIGN_STATUS name, "solved", and
        "inliers", an int32 array per correspondence of the group (1 / 0 for the records of a solved group, -1 for
        correspondences that were no records and for groups that are not solved)."""
        from .capi import SgAlignOptions, SgAlignResult
        gs = [np.ascontiguousarray(g, dtype=np.int32).reshape(-1, 2) for g in groups]
        n = len(gs)
        off = np.zeros(n + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(g) for g in gs])
        total = int(off[n])
        corr = np.concatenate(gs).reshape(-1) if total else np.zeros(0, dtype=np.int32)
        solved = np.zeros(n, dtype=np.int32)
        res = (SgAlignResult * max(n, 1))()
        inl = np.full(max(total, 1), -1, dtype=np.int32)
        opt = SgAlignOptions(threshold=threshold, max_hypotheses=max_hypotheses, min_inliers=min_inliers, seed=seed,
                             refine=int(bool(refine)), fix_scale=int(bool(fix_scale)), max_scale=max_scale,
                             min_gap=min_gap)
        ms = m.struct()
        ip = C.POINTER(C.c_int32)
        # (corr is passed by address even when empty: only its length decides whether it is read)
        check(self.lib.sg_slam_align_points(self.h, C.byref(ms), corr.ctypes.data_as(ip), off.ctypes.data_as(ip), n,
                                            C.byref(opt), solved.ctypes.data_as(ip), res, inl.ctypes.data_as(ip)),
              "Slam::AlignPoints")
        out = []
        for i in range(n):
            d = res[i].as_dict()
            d["solved"] = bool(solved[i])
            d["inliers"] = inl[off[i]:off[i + 1]].copy()
            out.append(d)
        return out

    def MatchByProjection(self, m: MapArrays, frames, keypoints, points, point_desc, radius_px: float = 12.0,
                          max_dist: int = 64, ratio_percent: int = 80, skip_observed: bool = True, width: int = 0,
                          height: int = 0) -> list:
        """Match by projection (sg_slam_match_by_projection): which of the listed map points does each listed frame
        see at its pose in m?  keypoints holds one (pixels (k, 2) float64, descriptors (k, 4) uint64) pair per listed
        frame; point_desc the (len(points), 4) uint64 descriptors of the listed points.  The points are projected into
        each frame on the device and a keypoint is compared only with the points inside radius_px of it; the accepted,
        unique matches (max_dist, the ratio test at ratio_percent) come back as one int32 array per frame: a map point
        index or -1 per keypoint.  With skip_observed, a point the frame already observes is no candidate; width and
        height, when given, cull projections outside the image.  The map is not written.
        projection_match_results() has the detail arrays and the per-frame counts."""
        from .capi import SgMatchOptions, SgMatchResult
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        n = len(fr)
        if len(keypoints) != n:
            raise ValueError("one (pixels, descriptors) pair per listed frame")
        xys = [np.ascontiguousarray(k[0], dtype=np.float64).reshape(-1, 2) for k in keypoints]
        dss = [np.ascontiguousarray(k[1], dtype=np.uint64).reshape(-1, 4) for k in keypoints]
        if any(len(a) != len(b) for a, b in zip(xys, dss)):
            raise ValueError("one descriptor per keypoint")
        off = np.zeros(n + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(a) for a in xys])
        K = int(off[n])
        xy = np.concatenate(xys).reshape(-1) if K else np.zeros(0)
        ds = np.concatenate(dss).reshape(-1) if K else np.zeros(0, dtype=np.uint64)
        pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1)
        pd = np.ascontiguousarray(point_desc, dtype=np.uint64).reshape(-1)
        if len(pd) != 4 * len(pts):
            raise ValueError("one descriptor per listed point")
        out = [np.full(max(K, 1), 7, dtype=np.int32) for _ in range(5)]
        res = (SgMatchResult * max(n, 1))()
        opt = SgMatchOptions(radius_px=radius_px, width=width, height=height, max_dist=max_dist,
                             ratio_percent=ratio_percent, skip_observed=int(bool(skip_observed)))
        ms = m.struct()
        ip, dp, up = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)
        # (empty arrays are passed by address: only the counts decide whether they are read)
        check(self.lib.sg_slam_match_by_projection(
            self.h, C.byref(ms), fr.ctypes.data_as(ip), n, off.ctypes.data_as(ip), xy.ctypes.data_as(dp),
            ds.ctypes.data_as(up), pts.ctypes.data_as(ip), len(pts), pd.ctypes.data_as(up), C.byref(opt),
            *[a.ctypes.data_as(ip) for a in out], res), "Slam::MatchByProjection")
        names = ("match", "best_point", "best_dist", "second_dist", "num_candidates")
        self._match_results = []
        for i in range(n):
            d = res[i].as_dict()
            for name, a in zip(names, out):
                d[name] = a[off[i]:off[i + 1]].copy()
            self._match_results.append(d)
        return [d["match"].copy() for d in self._match_results]

    def projection_match_results(self) -> list:
        """Result dicts of the last MatchByProjection call, one per listed frame: num_keypoints, num_projected,
        num_with_candidates, num_matched and the per-keypoint int32 arrays match, best_point, best_dist, second_dist
        and num_candidates."""
        return list(getattr(self, "_match_results", []))

    def MatchEpipolar(self, m: MapArrays, pairs, keypoints_a, keypoints_b, tol_px: float = 2.0,
                      min_parallax: float = 0.0, max_dist: int = 64, ratio_percent: int = 80) -> list:
        """Match along epipolar lines (sg_slam_match_epipolar): which keypoints of frame a and frame b of each listed
        pair (rows of pairs: frame a, frame b) are the same new landmark, at the poses in m?  keypoints_a and
        keypoints_b hold one (pixels (k, 2) float64, descriptors (k, 4) uint64[, levels (k,) int32]) tuple per pair:
        the keypoints of that frame the caller has not matched yet; levels are given for every tuple or for none.  An
        a keypoint is compared only with the b keypoints within tol_px (ideal pixels, Sampson, scaled by 2^level) of
        its epipolar line that triangulate in front of both cameras and, with min_parallax > 0 (rad), at that
        parallax or more.  The accepted, unique matches (max_dist, the ratio test at ratio_percent) come back as one
        int32 array per pair: per a keypoint, a b keypoint's index within the pair or -1.  The map is not written.
        epipolar_match_results() has the detail arrays and the per-pair counts."""
        self._epipolar_results = _match_epipolar(
            lambda *a: self.lib.sg_slam_match_epipolar(self.h, *a), m, pairs, keypoints_a, keypoints_b, tol_px,
            min_parallax, max_dist, ratio_percent, "Slam::MatchEpipolar")
        return [d["match"].copy() for d in self._epipolar_results]

    def epipolar_match_results(self) -> list:
        """Result dicts of the last MatchEpipolar call, one per listed pair: num_a, num_b, num_with_candidates,
        num_matched, degenerate and the per-a-keypoint int32 arrays match, best_kp, best_dist, second_dist and
        num_candidates."""
        return list(getattr(self, "_epipolar_results", []))

    def ApplySimilarity(self, m: MapArrays, scale: float, q, t, frames, points) -> None:
        """sg_map_apply_similarity: moves the listed frames and points of m through Y = scale R(q) X + t in place (on
        the host; pixels of moved frames on moved points do not change)."""
        qq = np.ascontiguousarray(q, dtype=np.float64).reshape(4)
        tt = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        pt = np.ascontiguousarray(points, dtype=np.int32).reshape(-1)
        ms = m.struct()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        check(self.lib.sg_map_apply_similarity(C.byref(ms), float(scale), qq.ctypes.data_as(dp), tt.ctypes.data_as(dp),
                                               fr.ctypes.data_as(ip), len(fr), pt.ctypes.data_as(ip), len(pt)),
              "Slam::ApplySimilarity")

    def PoseEdges(self, m: MapArrays, pairs, sim=None) -> np.ndarray:
        """sg_map_pose_edges: the (n, 8) measurements q^ (4), u^ (3), rho^ of the listed frame pairs (a, b) as the map
        stands (on the host; the map is not written).  sim = (scale, q, t), an AlignPoints result from a's piece to
        b's, makes loop edges: frame a is taken as ApplySimilarity would leave it, at local scale `scale`."""
        pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        meas = np.zeros((len(pr), 8))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        sm = None
        if sim is not None:
            sm = np.concatenate([[float(sim[0])], np.asarray(sim[1], dtype=np.float64).reshape(4),
                                 np.asarray(sim[2], dtype=np.float64).reshape(3)])
        ms = m.struct()
        check(self.lib.sg_map_pose_edges(C.byref(ms), pr.ctypes.data_as(ip), len(pr),
                                         sm.ctypes.data_as(dp) if sm is not None else None, meas.ctypes.data_as(dp)),
              "Slam::PoseEdges")
        return meas

    def CovisiblePairs(self, m: MapArrays, frames, min_shared: int) -> np.ndarray:
        """sg_map_covisible_pairs: the (K, 2) pairs (i < j, positions in `frames`, lexicographic) of listed frames that
        share at least min_shared slam-usable points through enabled observations (on the host)."""
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        ip = C.POINTER(C.c_int32)
        cnt = C.c_int32()
        ms = m.struct()
        check(self.lib.sg_map_covisible_pairs(C.byref(ms), fr.ctypes.data_as(ip), len(fr), int(min_shared), None, 0,
                                              C.byref(cnt)), "Slam::CovisiblePairs")
        out = np.zeros((max(cnt.value, 1), 2), dtype=np.int32)
        check(self.lib.sg_map_covisible_pairs(C.byref(ms), fr.ctypes.data_as(ip), len(fr), int(min_shared),
                                              out.ctypes.data_as(ip), cnt.value, C.byref(cnt)), "Slam::CovisiblePairs")
        return out[:cnt.value]

    def OptimizePoseGraph(self, m: MapArrays, graphs, range_: float = 0.0, fix_scale: bool = False,
                          move_points: bool = False, cpu: bool = False, options=None) -> list:
        """Pose-graph optimisation (sg_slam_optimize_pose_graph): spreads loop closures over the frames.  Each graph
        is a dict with "frames" (map frame indices), "fixed" (one flag per node), "edges" ((E, 2) positions a, b in
        the node list), "meas" ((E, 8): q^, u^, rho^ as PoseEdges gives them) and "weights" ((E, 3): w_rot, w_t,
        w_s).  All graphs of a call run in one device launch, one workgroup each.  Updates m.q / m.t of the free nodes
        of the solved graphs in place (and m.X with move_points).  Returns one dict per graph: "status" (a PG_STATUS
        name), "log_scale" (one per node) and the fields of its solver summary.  cpu=True solves the same call with
        the planner's CPU executor on the host instead (a development aid: no handle, no device; `options`, an
        SgSolverOptions, defaults to default_solver_options())."""
        from .capi import PG_STATUS, SgPosegraphOptions, default_solver_options
        n = len(graphs)
        noff = np.zeros(n + 1, dtype=np.int32)
        eoff = np.zeros(n + 1, dtype=np.int32)
        fr, fx, ab, meas, wts = [], [], [], [], []
        for i, g in enumerate(graphs):
            fr.append(np.asarray(g["frames"], dtype=np.int32).reshape(-1))
            fx.append(np.asarray(g["fixed"], dtype=np.int32).reshape(-1))
            ab.append(np.asarray(g["edges"], dtype=np.int32).reshape(-1, 2))
            meas.append(np.asarray(g["meas"], dtype=np.float64).reshape(-1, 8))
            wts.append(np.asarray(g["weights"], dtype=np.float64).reshape(-1, 3))
            if not (len(fr[i]) == len(fx[i]) and len(ab[i]) == len(meas[i]) == len(wts[i])):
                raise ValueError("graph %d: list lengths differ" % i)
            noff[i + 1] = noff[i] + len(fr[i])
            eoff[i + 1] = eoff[i] + len(ab[i])
        cat = lambda v, dt, w: (np.ascontiguousarray(np.concatenate(v), dtype=dt) if n else np.zeros((0, w), dtype=dt))
        fr_, fx_ = cat(fr, np.int32, 1).reshape(-1), cat(fx, np.int32, 1).reshape(-1)
        ab_, meas_, wts_ = cat(ab, np.int32, 2), cat(meas, np.float64, 8), cat(wts, np.float64, 3)
        status = np.zeros(max(n, 1), dtype=np.int32)
        ls = np.zeros(max(int(noff[n]), 1))
        sums = (SgSolverSummary * max(n, 1))()
        opt = SgPosegraphOptions(range=range_, fix_scale=int(bool(fix_scale)), move_points=int(bool(move_points)))
        ms = m.struct()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        lists = (fr_.ctypes.data_as(ip), fx_.ctypes.data_as(ip), noff.ctypes.data_as(ip), ab_.ctypes.data_as(ip),
                 meas_.ctypes.data_as(dp), wts_.ctypes.data_as(dp), eoff.ctypes.data_as(ip), n, C.byref(opt))
        if cpu:
            so = options if options is not None else default_solver_options()
            fn = self.lib.sg_posegraph_debug_cpu_solve
            fn.restype = C.c_int
            fn.argtypes = [C.POINTER(type(ms)), ip, ip, ip, ip, dp, dp, ip, C.c_int32, C.POINTER(SgPosegraphOptions),
                           C.POINTER(type(so)), ip, dp, C.POINTER(SgSolverSummary)]
            check(fn(C.byref(ms), *lists, C.byref(so), status.ctypes.data_as(ip), ls.ctypes.data_as(dp), sums),
                  "sg_posegraph_debug_cpu_solve")
        else:
            check(self.lib.sg_slam_optimize_pose_graph(self.h, C.byref(ms), *lists, status.ctypes.data_as(ip),
                                                       ls.ctypes.data_as(dp), sums), "Slam::OptimizePoseGraph")
        out = []
        for i in range(n):
            d = sums[i].as_dict()
            d["status"] = PG_STATUS.get(int(status[i]), "?")
            d["log_scale"] = ls[noff[i]:noff[i + 1]].copy()
            out.append(d)
        return out

    def SolvePoints(self, m: MapArrays, points, range_: float) -> list:
        """Structure-only bundle adjustment (sg_slam_solve_points): each listed point's location against the map's
        frames as they are, all points in one device launch.  Point flags are not consulted.  Updates m.X of the
        solved points in place and returns one bool per listed point; point_summaries() has their summaries."""
        pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1)
        n = len(pts)
        solved = np.zeros(n, dtype=np.int32)
        sums = (SgSolverSummary * max(n, 1))()
        ms = m.struct()
        check(self.lib.sg_slam_solve_points(self.h, C.byref(ms), pts.ctypes.data_as(C.POINTER(C.c_int32)), n, range_,
                                            solved.ctypes.data_as(C.POINTER(C.c_int32)), sums),
              "Slam::SolvePoints")
        self._point_summaries = [sums[i].as_dict() for i in range(n)]
        return [bool(v) for v in solved]

    def point_summaries(self) -> list:
        """Summary dicts of the last SolvePoints or TriangulatePoints call, one per listed point."""
        return list(getattr(self, "_point_summaries", []))

    def TriangulatePoints(self, m: MapArrays, points, min_parallax: float = 0.0, max_error_px: float = 0.0,
                          refine: bool = False, range_: float = 2.0) -> list:
        """Linear multi-view triangulation (sg_slam_triangulate_points): each listed point's location from its
        enabled observations alone, against the map's frames as they are, all points in one device launch.  The
        location at entry is not read; point flags are not consulted.  min_parallax (rad) and max_error_px gate
        the result, 0 = off; refine polishes the accepted points with SolvePoints' solver (CauchyLoss(range_)) on
        the device.  Updates m.X of the accepted points in place and returns one bool per listed point;
        triangulation_results() has their statuses and quality figures, point_summaries() the polish's."""
        pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1)
        n = len(pts)
        solved = np.zeros(n, dtype=np.int32)
        res = (SgTriangulateResult * max(n, 1))()
        sums = (SgSolverSummary * max(n, 1))()
        opt = SgTriangulateOptions(min_parallax=min_parallax, max_error_px=max_error_px, refine=int(bool(refine)),
                                   range=range_)
        ms = m.struct()
        check(self.lib.sg_slam_triangulate_points(self.h, C.byref(ms), pts.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                                  C.byref(opt), solved.ctypes.data_as(C.POINTER(C.c_int32)), res,
                                                  sums), "Slam::TriangulatePoints")
        self._triangulation_results = [res[i].as_dict() for i in range(n)]
        self._point_summaries = [sums[i].as_dict() for i in range(n)]
        return [bool(v) for v in solved]

    def triangulation_results(self) -> list:
        """Result dicts of the last TriangulatePoints call, one per listed point: status (a TRI_STATUS name),
        num_obs, parallax (rad), max_error_px, rel_gap and the triangulated X (before the polish)."""
        return list(getattr(self, "_triangulation_results", []))

    def ReprojectMap(self, m: MapArrays) -> float:
        mean = C.c_double()
        ms = m.struct()
        check(self.lib.sg_slam_reproject_map(self.h, C.byref(ms), C.byref(mean)), "Slam::ReprojectMap")
        return mean.value

    # LocalMap maintenance (localmap.cpp), on the device through the same handle.  These mirror
    # LocalMap::Clean / LocalMap::ApplyEpipolarConstraint, which main.cpp calls after each solve.
    def Clean(self, m: MapArrays, error_threshold: float) -> bool:
        """LocalMap::Clean (localmap.cpp:283-398) on m's ReprojectMap residuals; mutates m in place."""
        res = C.c_int32()
        ms = m.struct()
        check(self.lib.sg_map_clean(self.h, C.byref(ms), error_threshold, C.byref(res)), "LocalMap::Clean")
        return bool(res.value)

    def ApplyEpipolarConstraint(self, m: MapArrays) -> int:
        """LocalMap::ApplyEpipolarConstraint (localmap.cpp:232-276); mutates m.  Returns the violation count."""
        n = C.c_int32()
        ms = m.struct()
        check(self.lib.sg_map_apply_epipolar(self.h, C.byref(ms), C.byref(n)), "LocalMap::ApplyEpipolarConstraint")
        return n.value

    def Normalize(self, m: MapArrays):
        """LocalMap::Normalize (localmap.cpp:114-155) on the device; mutates m's poses and points in place."""
        ms = m.struct()
        check(self.lib.sg_map_normalize(self.h, C.byref(ms)), "LocalMap::Normalize")

    def iterations(self) -> int:
        return int(self.lib.sg_slam_iterations(self.h))

    def load_counts(self) -> tuple:
        """(full loads, value-only loads) of SolveFrames / SolveAllFrames calls on this object."""
        full, vals = C.c_int32(0), C.c_int32(0)
        check(self.lib.sg_slam_load_counts(self.h, C.byref(full), C.byref(vals)), "sg_slam_load_counts")
        return full.value, vals.value

    def last_phase_ms(self) -> dict:
        """Host wall time of the last SolveFrames / SolveAllFrames call by phase (ms)."""
        v = (C.c_double * 4)()
        check(self.lib.sg_slam_last_phase_ms(self.h, v), "sg_slam_last_phase_ms")
        return {"setup": v[0], "load": v[1], "solve": v[2], "write_back": v[3]}

    def error(self) -> float:
        return float(self.lib.sg_slam_error(self.h))

    def last_summary(self) -> dict:
        s = SgSolverSummary()
        check(self.lib.sg_slam_last_summary(self.h, C.byref(s)), "sg_slam_last_summary")
        return s.as_dict()
