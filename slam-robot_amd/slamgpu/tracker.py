"""Device HessianTracker (hessian.h) and the matcher's forward/backward step (matcher.cpp:173-206, 247-251)
behind the C-ABI (include/slamgpu.h, sg_tracker_*).

Method names follow the reference: MakePyramid builds a view's pyramid (into a device slot), GetPatch /
GetPatches sample patches, TrackFeatureFB is matcher.cpp's TrackFeature (forward + backward + 0.3 px check)
including FindMatches' retry with 6 levels.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .capi import SgDetectLevel, SgDetectOptions, SgDeviceOptions, SgTrackerOptions, check, load_library


def _dev(device=0):
    return SgDeviceOptions(device=device, precision=0, rank=0, nranks=1)

_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)
_dp = C.POINTER(C.c_double)


def default_tracker_options(**kw) -> SgTrackerOptions:
    lib = load_library()
    o = SgTrackerOptions()
    lib.sg_tracker_options_default(C.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def describe_call(fn, handle, key: int, xy, levels, what: str):
    """sg_tracker_describe / sg_frontend_describe (`key` = slot / frame): (desc uint64 (n, 4), angle_bin, status)."""
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    n = xy.shape[0]
    lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.int32).reshape(-1)
    if lv is not None and lv.shape[0] != n:
        raise ValueError("one level per keypoint")
    desc = np.zeros((n, 4), np.uint64)
    ang = np.zeros(n, np.int32)
    st = np.zeros(n, np.int32)
    check(fn(handle, key, n, xy.ctypes.data_as(_fp), None if lv is None else lv.ctypes.data_as(_ip),
             desc.ctypes.data_as(C.POINTER(C.c_uint64)), ang.ctypes.data_as(_ip), st.ctypes.data_as(_ip)), what)
    return desc, ang, st


def default_detect_options(**kw) -> SgDetectOptions:
    lib = load_library()
    o = SgDetectOptions()
    lib.sg_detect_options_default(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError("no detect option %r" % k)
        setattr(o, k, v)
    return o


def detect_cap(w: int, h: int, depth: int, per_cell: int) -> int:
    """What always holds every keypoint: the 32 x 32 cells of all `depth` levels of a w x h image, times per_cell."""
    cells = 0
    for _ in range(depth):
        cells += ((w + 31) // 32) * ((h + 31) // 32)
        w, h = (w + 1) // 2, (h + 1) // 2
    return cells * per_cell


def detect_call(fn, handle, key: int, w: int, h: int, depth: int, options: dict, what: str):
    """sg_tracker_detect / sg_frontend_detect (`key` = slot / frame) on a pyramid of `depth` levels over a w x h
    image: (xy float32 (n, 2) level-0 pixels, levels int32 (n), score float32 (n), per_level list of dicts)."""
    o = default_detect_options(**options)
    cap = detect_cap(w, h, depth, max(1, min(16, o.per_cell)))
    xy = np.zeros((cap, 2), np.float32)
    lv = np.zeros(cap, np.int32)
    sc = np.zeros(cap, np.float32)
    n = C.c_int32()
    per = (SgDetectLevel * depth)()
    check(fn(handle, key, C.byref(o), cap, xy.ctypes.data_as(_fp), lv.ctypes.data_as(_ip), sc.ctypes.data_as(_fp),
             C.byref(n), per), what)
    k = min(n.value, cap)
    return xy[:k].copy(), lv[:k].copy(), sc[:k].copy(), [p.as_dict() for p in per]


class HessianTracker:
    def __init__(self, window: int = 13, depth: int = 6, device: int = 0, max_images: int = 8, **kw):
        self.lib = load_library()
        self.opt = default_tracker_options(window=window, depth=depth, max_images=max_images, **kw)
        self.h = C.c_void_p()
        dev = _dev(device)
        check(self.lib.sg_tracker_create(C.byref(self.h), C.byref(self.opt), C.byref(dev)), "sg_tracker_create")

    def close(self):
        if self.h:
            self.lib.sg_tracker_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def window(self) -> int:
        return self.opt.window

    def MakePyramid(self, img: np.ndarray, slot: int = 0):
        """hessian.h:95-126.  img: (h, w, 3) uint8 in cv::Mat (BGR) memory order."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        h, w = img.shape[:2]
        check(self.lib.sg_tracker_set_image(self.h, slot, img.ctypes.data_as(_u8p), w, h, img.strides[0]),
              "sg_tracker_set_image")
        return slot

    def level(self, slot: int, level: int) -> np.ndarray:
        w, h = C.c_int32(), C.c_int32()
        check(self.lib.sg_tracker_get_level(self.h, slot, level, None, C.byref(w), C.byref(h)), "get_level")
        out = np.zeros((h.value, w.value), np.float32)
        check(self.lib.sg_tracker_get_level(self.h, slot, level, out.ctypes.data_as(_fp), C.byref(w), C.byref(h)),
              "get_level")
        return out

    def GetPatches(self, slot: int, level: int, xy: np.ndarray):
        """GetPatch (hessian.h:54-93) at many points: (patches[n, W, W], mean[n], sumsq[n])."""
        xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
        n, W = xy.shape[0], self.window
        out = np.zeros((n, W, W), np.float32)
        mean = np.zeros(n, np.float32)
        sumsq = np.zeros(n, np.float32)
        check(self.lib.sg_tracker_get_patches(self.h, slot, level, n, xy.ctypes.data_as(_fp), out.ctypes.data_as(_fp),
                                              mean.ctypes.data_as(_fp), sumsq.ctypes.data_as(_fp)), "get_patches")
        return out, mean, sumsq

    def TrackFeatureFB(self, from_slot: int, to_slot: int, from_xy, to_xy=None, levels=None):
        """matcher.cpp TrackFeature for many features.  Returns (to_xy, accepted[bool], iterations)."""
        from_xy = np.ascontiguousarray(from_xy, dtype=np.float32).reshape(-1, 2)
        n = from_xy.shape[0]
        out = (from_xy.copy() if to_xy is None else np.ascontiguousarray(to_xy, dtype=np.float32).reshape(-1, 2).copy())
        lv = np.full(n, 3, np.int32) if levels is None else np.ascontiguousarray(levels, dtype=np.int32)
        acc = np.zeros(n, np.int32)
        its = np.zeros(n, np.int32)
        check(self.lib.sg_tracker_track(self.h, from_slot, to_slot, n, from_xy.ctypes.data_as(_fp),
                                        out.ctypes.data_as(_fp), lv.ctypes.data_as(_ip), acc.ctypes.data_as(_ip),
                                        its.ctypes.data_as(_ip)), "sg_tracker_track")
        return out, acc.astype(bool), its

    # device-resident throughput path (bench)
    def load_features(self, from_xy, to_xy, levels=None):
        from_xy = np.ascontiguousarray(from_xy, dtype=np.float32).reshape(-1, 2)
        to_xy = np.ascontiguousarray(to_xy, dtype=np.float32).reshape(-1, 2)
        n = from_xy.shape[0]
        lv = np.full(n, 3, np.int32) if levels is None else np.ascontiguousarray(levels, dtype=np.int32)
        self._n = n
        check(self.lib.sg_tracker_load_features(self.h, n, from_xy.ctypes.data_as(_fp), to_xy.ctypes.data_as(_fp),
                                                lv.ctypes.data_as(_ip)), "load_features")

    def run(self, from_slot: int, to_slot: int, repeats: int = 1):
        check(self.lib.sg_tracker_run(self.h, from_slot, to_slot, repeats), "sg_tracker_run")

    def results(self):
        n = self._n
        out = np.zeros((n, 2), np.float32)
        acc = np.zeros(n, np.int32)
        its = np.zeros(n, np.int32)
        check(self.lib.sg_tracker_results(self.h, out.ctypes.data_as(_fp), acc.ctypes.data_as(_ip),
                                          its.ctypes.data_as(_ip)), "sg_tracker_results")
        return out, acc.astype(bool), its

    def kernel_ms(self):
        t, p = C.c_double(), C.c_double()
        check(self.lib.sg_tracker_kernel_ms(self.h, C.byref(t), C.byref(p)), "kernel_ms")
        return t.value, p.value

    def Describe(self, slot: int, xy, levels=None):
        """Oriented 256-bit descriptors (sg_tracker_describe) of the keypoints xy (n, 2), level-0 pixels, each on
        pyramid level levels[i] (None = level 0) of `slot`.  Returns (desc uint64 (n, 4), angle_bin (n), status (n):
        0 OK, 1 BORDER with a zero descriptor and angle_bin -1); the rows feed hamming_match / MatchByProjection."""
        return describe_call(self.lib.sg_tracker_describe, self.h, slot, xy, levels, "sg_tracker_describe")

    def describe_ms(self) -> float:
        """Kernel time of the last Describe launch (HIP events)."""
        ms = C.c_double()
        check(self.lib.sg_tracker_describe_ms(self.h, C.byref(ms)), "sg_tracker_describe_ms")
        return ms.value

    def Detect(self, slot: int, **options):
        """FAST-9 keypoints (sg_tracker_detect) on the pyramid of `slot`, spread by 32 x 32 cells; options are
        sg_detect_options' fields (threshold, min_threshold, first_level, num_levels, border, per_cell,
        max_keypoints).  Returns (xy (n, 2) level-0 pixels, levels (n), score (n), per_level: one dict per pyramid
        level); xy and levels go straight into Describe."""
        w, h = C.c_int32(), C.c_int32()
        check(self.lib.sg_tracker_get_level(self.h, slot, 0, None, C.byref(w), C.byref(h)), "get_level")
        return detect_call(self.lib.sg_tracker_detect, self.h, slot, w.value, h.value, self.opt.depth, options,
                           "sg_tracker_detect")

    def detect_ms(self) -> float:
        """Kernel time of the last Detect launch (HIP events)."""
        ms = C.c_double()
        check(self.lib.sg_tracker_detect_ms(self.h, C.byref(ms)), "sg_tracker_detect_ms")
        return ms.value

    def DetectAndDescribe(self, slot: int, **options):
        """Detect, then Describe on the result; only the keypoints whose descriptor is SG_DESC_OK are returned
        (with the default border of 15 that is all of them): (xy, levels, score, desc uint64 (n, 4), angle_bin)."""
        xy, lv, sc, _ = self.Detect(slot, **options)
        desc, ang, st = self.Describe(slot, xy, lv)
        ok = st == 0
        return xy[ok], lv[ok], sc[ok], desc[ok], ang[ok]

    def TrackFeature(self, from_slot: int, to_slot: int, from_xy, to_xy=None, levels=None):
        """One-directional TrackFeature of this tracker's mode (hessian.h:243-264 / klt.h:403-424 /
        brute.h:129-164) for many features: GetPatches(from_slot, from_xy), then tracking in to_slot from to_xy.
        Returns (to_xy, status (0 OK, 2 OUT_OF_BOUNDS), iterations); failed features keep their guess."""
        from_xy = np.ascontiguousarray(from_xy, dtype=np.float32).reshape(-1, 2)
        n = from_xy.shape[0]
        out = (from_xy.copy() if to_xy is None else np.ascontiguousarray(to_xy, dtype=np.float32).reshape(-1, 2).copy())
        lv = None if levels is None else np.ascontiguousarray(levels, dtype=np.int32)
        st = np.zeros(n, np.int32)
        its = np.zeros(n, np.int32)
        check(self.lib.sg_tracker_track_feature(self.h, from_slot, to_slot, n, from_xy.ctypes.data_as(_fp),
                                                out.ctypes.data_as(_fp), None if lv is None else lv.ctypes.data_as(_ip),
                                                st.ctypes.data_as(_ip), its.ctypes.data_as(_ip)),
              "sg_tracker_track_feature")
        return out, st, its

    def SeedFeatures(self, slot: int, match_xy=None, max_corners: int = 120, quality: float = 0.01,
                     min_distance: float = 20.0):
        """Matcher::Track's new-keyframe seeding on the image of `slot` (matcher.cpp:123-169, AddNewFeatures):
        goodFeaturesToTrack(grey, 120, 0.01, 20) then the 30 x 30 grid filter against the current matches.
        Returns (corners[n, 2], added[m, 2])."""
        mxy = np.ascontiguousarray(np.zeros((0, 2)) if match_xy is None else match_xy, dtype=np.float32).reshape(-1, 2)
        corners = np.zeros((max_corners, 2), np.float32)
        added = np.zeros((max_corners, 2), np.float32)
        nc, na = C.c_int32(), C.c_int32()
        check(self.lib.sg_tracker_seed_features(self.h, slot, mxy.ctypes.data_as(_fp) if len(mxy) else None, len(mxy),
                                                max_corners, quality, min_distance, corners.ctypes.data_as(_fp),
                                                C.byref(nc), added.ctypes.data_as(_fp), C.byref(na)),
              "sg_tracker_seed_features")
        return corners[:nc.value].copy(), added[:na.value].copy()


class KLTTracker(HessianTracker):
    """klt.h's KLTTracker on the device (sg_tracker_options.mode = SG_TRACKER_KLT): MakePyramid and
    TrackFeature with klt.h's pyramid, masked SSD and forward-difference Newton step."""

    def __init__(self, window: int = 13, depth: int = 6, device: int = 0, max_images: int = 8, **kw):
        super().__init__(window=window, depth=depth, device=device, max_images=max_images, mode=1, **kw)


class BruteTracker(HessianTracker):
    """brute.h's BruteTracker on the device (sg_tracker_options.mode = SG_TRACKER_BRUTE): exhaustive
    float-stepped SearchBest grids, one candidate per thread."""

    def __init__(self, window: int = 13, depth: int = 6, device: int = 0, max_images: int = 8, **kw):
        super().__init__(window=window, depth=depth, device=device, max_images=max_images, mode=2, **kw)
