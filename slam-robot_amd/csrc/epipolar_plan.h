// epipolar_plan.h — the host-only planner of sg_slam_match_epipolar (ba_epipolar.hip): from an sg_map, the listed frame
// pairs with their keypoint counts and the options, everything the three kernels read, the launch shapes, the rule that
// turns the downloaded arrays into matches, and a plain CPU executor of the whole contract.  Pure functions of their
// arguments (no HIP, no environment, no state, no I/O), so a CPU test recomputes them by brute force
// (tests/native/epipolar_plan_check.cpp).
//
// Per listed pair: its record (epipolar_math.h).  A pair is live when it is not degenerate and has keypoints on both
// sides; only live pairs give work.  The preparation list: one item per (live pair, side, run of kEpiPrepRun
// keypoints).  The work list: one item per (live pair, chunk of kEpiChunk a keypoints, slice of kEpiSlice b keypoints).
// The merge list: one item per (live pair, chunk).  Every count is known on the host, so the device keeps no counter
// and uses no atomic.  The partial results of pair i, 16 bytes per (a keypoint, slice), lie at part0_i + s * na_i + k
// (k the a keypoint's index within the pair) with part0_i the sum over the earlier live pairs of na * slices.
#ifndef SG_EPIPOLAR_PLAN_H_
#define SG_EPIPOLAR_PLAN_H_

#include <cstdint>
#include <vector>

#include "best2.h"
#include "epipolar_math.h"
#include "slamgpu.h"

namespace sg {

constexpr int kEpiChunk = 64;             // a keypoints per workgroup of k_epi_window (one per lane of each wave)
constexpr int kEpiTile = 256;             // b keypoints staged in LDS at a time (one per thread, a quarter per wave)
constexpr int kEpiSlice = 512;            // b keypoints per workgroup of k_epi_window: a whole number of tiles
constexpr int kEpiPrepRun = 256;          // keypoints per workgroup of k_epi_prep
constexpr int kEpiMaxKeypoints = 1 << 20;
constexpr int kEpiKeyShift = kBest2Shift; // the packed key: (distance << 22) | b index within the pair (best2.h)
constexpr int64_t kEpiMaxPartials = (int64_t)1 << 23;   // 16 bytes each: 128 MiB
constexpr int kEpiMaxLevel = 7;
static_assert(kEpiSlice % kEpiTile == 0, "a slice is whole tiles");
static_assert(kEpiMaxKeypoints <= (1 << kEpiKeyShift), "a b index fits the key");

struct EpiPrepItem {
  int32_t pair;    // the listed pair: an index into the call's pairs
  int32_t side;    // 0: a keypoints, 1: b keypoints
  int32_t k0;      // first keypoint of the run, an index into the call's a (or b) keypoints
  int32_t count;   // 1 .. kEpiPrepRun
};
static_assert(sizeof(EpiPrepItem) == 16, "read by k_epi_prep as 4 ints");

struct EpiItem {
  int32_t pair;
  int32_t a0, acount;   // the chunk: first a keypoint (an index into the call's a keypoints), 1 .. kEpiChunk
  int32_t b0, bcount;   // the slice: first b keypoint (an index into the call's b keypoints), 1 .. kEpiSlice
  int32_t j0;           // b0's index within the pair
  int32_t part0;        // where lane 0's partial result goes
  int32_t pad;
};
static_assert(sizeof(EpiItem) == 32, "read by k_epi_window as 8 ints");

struct EpiChunkItem {
  int32_t a0, count;    // the chunk
  int32_t part0;        // lane 0's partial result of slice 0
  int32_t stride;       // the pair's a keypoints: from one slice's partial results to the next
  int32_t slices;       // 1 ..
  int32_t pad[3];
};
static_assert(sizeof(EpiChunkItem) == 32, "read by k_epi_merge as 8 ints");

struct EpipolarPlan {
  int32_t n = 0, KA = 0, KB = 0;
  bool levels = false;
  std::vector<EpiPair> pairs;           // [n]
  std::vector<uint8_t> live;            // [n]
  std::vector<EpiPrepItem> prep;
  std::vector<EpiItem> items;           // pairs in listed order, chunks in keypoint order, slices in order
  std::vector<EpiChunkItem> chunks;
  int64_t partials = 0;                 // over the live pairs
  bool launch = false;                  // a live pair exists
};

// Throws sg::Error(SG_EINVAL) on every argument error of sg_slam_match_epipolar's contract that concerns the map, the
// lists and the options (the handle and the output arrays are the caller's).  n == 0 gives an empty plan (the lists are
// then not read and may be null).
void PlanEpipolar(const sg_map* m, const int32_t* pairs, int32_t n, const int32_t* a_offset, const double* a_xy,
                  const uint64_t* a_desc, const int32_t* a_level, const int32_t* b_offset, const double* b_xy,
                  const uint64_t* b_desc, const int32_t* b_level, const sg_epipolar_options* o, EpipolarPlan* out);

// Step 5 of the contract: match[KA] and results[n] (may be null) from the per-keypoint arrays: ResolveMatches of
// match_plan.h applied per pair, with the b index within the pair as the claimed point.
void ResolveEpipolar(const EpipolarPlan& plan, const int32_t* a_offset, const int32_t* b_offset, const int32_t* best_kp,
                     const int32_t* best_dist, const int32_t* second_dist, const int32_t* num_candidates,
                     const sg_epipolar_options& o, int32_t* match, sg_epipolar_result* results);

// Steps 2 to 4 of the contract on one host thread, in plain loops: the four per-keypoint arrays [KA], all written
// (the empty answers for a pair that is not live).
void RunEpipolarCpu(const EpipolarPlan& plan, const int32_t* a_offset, const double* a_xy, const uint64_t* a_desc,
                    const int32_t* a_level, const int32_t* b_offset, const double* b_xy, const uint64_t* b_desc,
                    const int32_t* b_level, const sg_epipolar_options& o, int32_t* best_kp, int32_t* best_dist,
                    int32_t* second_dist, int32_t* num_candidates);

}  // namespace sg

#endif  // SG_EPIPOLAR_PLAN_H_
