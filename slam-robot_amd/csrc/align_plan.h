// align_plan.h — the host-only planner of sg_slam_align_points (ba_align.hip): from an sg_map, the groups of
// landmark correspondences and the options, everything the two kernels read, and the launch shape.  A pure function of
// its arguments (no HIP, no environment, no state, no I/O), so a CPU test recomputes it by brute force
// (tests/native/align_plan_check.cpp).
//
// Per group: its records (correspondences whose two points are slam-usable, finite and not at infinity, in listed
// order) as six doubles, X_a.xyz / X_a.w then X_b.xyz / X_b.w, with the index of the correspondence beside them; the
// sampler's key (the map index of point a of the group's first listed correspondence, 0 for an empty group); and
// whether it runs (4 records or more).
#ifndef SG_ALIGN_PLAN_H_
#define SG_ALIGN_PLAN_H_

#include <cstdint>
#include <vector>

#include "slamgpu.h"

namespace sg {

constexpr int kAlignMinRecords = 4;
constexpr int kAlignThreads = 256;             // hypotheses per workgroup of k_align_ransac
constexpr int kAlignMaxHypotheses = 1 << 20;
// A point with |W| < kAlignMinW |X|_2 is at infinity for this call (kPnpMinW of pnp_math.h, for any 4-norm).
constexpr double kAlignMinW = 1e-9;

struct AlignGroup {
  int32_t key;        // PnpSample's second argument
  int32_t run;        // 0: fewer than kAlignMinRecords records (SG_ALIGN_DID_NOT_RUN, no workgroup work)
  int32_t num_corr;   // correspondences listed
  int32_t pad;
};
static_assert(sizeof(AlignGroup) == 16, "read by the kernels as 4 ints");

struct AlignPlan {
  std::vector<int32_t> off;         // [n + 1] records of group g: off[g] .. off[g + 1]
  std::vector<double> records;      // [6 off[n]]
  std::vector<int32_t> rec_corr;    // [off[n]] the record's correspondence, an index into the call's list
  std::vector<AlignGroup> groups;   // [n]
  int num_run = 0;
  int H = 0, S = 0;                 // hypotheses per group, workgroups per group (H / kAlignThreads)
  int64_t grid = 0;                 // n * S workgroups
};

// Throws sg::Error(SG_EINVAL) on every argument error of sg_slam_align_points' contract that concerns the map, the
// lists and the options.  n == 0 gives an empty plan (the lists are then not read and may be null).
void PlanAlign(const sg_map* m, const int32_t* corr, const int32_t* group_offset, int32_t n,
               const sg_align_options* o, AlignPlan* out);

}  // namespace sg

#endif  // SG_ALIGN_PLAN_H_
