// match_plan.h — the host-only planner of sg_slam_match_by_projection (ba_match.hip): from an sg_map, the listed
// frames with their keypoints, the listed points and the options, everything the three kernels read, the launch
// shapes, and the rule that turns the downloaded arrays into matches.  Pure functions of their arguments (no HIP, no
// environment, no state, no I/O), so a CPU test recomputes them by brute force (tests/native/match_plan_check.cpp).
//
// Per listed frame: its pose and intrinsics as 14 doubles (q, t, k).  Per listed point, in listed order: its location.
// The skip_observed exclusion as one bit per (listed frame, position): n rows of ceil(np / 32) words.  The work list:
// one item per (listed frame, chunk of kMatchChunk keypoints).  The launch shapes come from upper bounds only (np, not
// the number of points that will project): the survivor counts stay on the device.
#ifndef SG_MATCH_PLAN_H_
#define SG_MATCH_PLAN_H_

#include <cstdint>
#include <vector>

#include "best2.h"
#include "slamgpu.h"

namespace sg {

constexpr int kMatchChunk = 64;            // keypoints per workgroup of k_match_window (one per lane of each wave)
constexpr int kMatchTile = 256;            // survivors staged in LDS at a time (one per thread, a quarter per wave)
constexpr int kMatchSlice = 512;           // survivors per workgroup of k_match_window: a whole number of tiles
constexpr int kMatchMaxKeypoints = 1 << 20;
constexpr int kMatchKeyShift = kBest2Shift;   // the packed key: (distance << 22) | position (best2.h)
constexpr int64_t kMatchMaxPairs = (int64_t)1 << kMatchKeyShift;   // n * np
static_assert(kMatchSlice % kMatchTile == 0, "a slice is whole tiles");

struct MatchFrame {
  double q[4], t[3], k[7];
};
static_assert(sizeof(MatchFrame) == 112, "read by k_match_project as 14 doubles");

struct MatchChunk {
  int32_t slot;    // the listed frame: an index into the call's frames[]
  int32_t kp0;     // first keypoint of the chunk, an index into the call's keypoints
  int32_t count;   // 1 .. kMatchChunk
  int32_t pad;
};
static_assert(sizeof(MatchChunk) == 16, "read by the kernels as 4 ints");

struct MatchPlan {
  int32_t n = 0, np = 0, K = 0;
  std::vector<MatchFrame> frames;    // [n]
  std::vector<double> X;             // [4 np] the listed points' locations, in listed order
  std::vector<uint32_t> excl;        // [n * words]; bit (j & 31) of word slot * words + (j >> 5): position j is excluded
  std::vector<MatchChunk> chunks;    // frames in listed order, chunks in keypoint order
  int32_t words = 0;                 // ceil(np / 32)
  int32_t slices = 0;                // ceil(np / kMatchSlice): the survivor slices a frame can have
  int32_t project_blocks = 0;        // ceil(np / 256): k_match_project runs project_blocks x n workgroups
  bool launch = false;               // K > 0 and np > 0
};

// Throws sg::Error(SG_EINVAL) on every argument error of sg_slam_match_by_projection's contract that concerns the map,
// the lists and the options (the handle and the output arrays are the caller's).  n == 0 gives an empty plan (the
// lists are then not read and may be null).
void PlanMatch(const sg_map* m, const int32_t* frames, int32_t n, const int32_t* kp_offset, const double* kp_xy,
               const uint64_t* kp_desc, const int32_t* points, int32_t np, const uint64_t* point_desc,
               const sg_match_options* o, MatchPlan* out);

// Step 3 of the contract: match[K] and the last two fields of results[n] from the per-keypoint arrays.  results may be
// null; num_keypoints and num_projected are not touched.
void ResolveMatches(const int32_t* kp_offset, int32_t n, const int32_t* best_point, const int32_t* best_dist,
                    const int32_t* second_dist, const int32_t* num_candidates, const sg_match_options& o,
                    int32_t* match, sg_match_result* results);

}  // namespace sg

#endif  // SG_MATCH_PLAN_H_
