// relpose_plan.h — the host-only planner of sg_slam_relative_poses (ba_relpose.hip): from an sg_map, a list of frame
// pairs and the options, everything the two kernels read, and the launch shape.  A pure function of its arguments (no
// HIP, no environment, no state, no I/O), so a CPU test recomputes it by brute force
// (tests/native/relpose_plan_check.cpp).
//
// Per pair (a, b): its records (points with an enabled observation in both frames, in the map order of a's
// observations, the first enabled observation of the point in each frame) as four doubles, pixel in a then pixel in b,
// with the two map observation indices beside them; both cameras' intrinsics; and whether it runs (8 records or more).
#ifndef SG_RELPOSE_PLAN_H_
#define SG_RELPOSE_PLAN_H_

#include <cstdint>
#include <vector>

#include "slamgpu.h"

namespace sg {

constexpr int kRelMinObs = 8;
constexpr int kRelThreads = 256;               // hypotheses per workgroup of k_relpose_ransac
constexpr int kRelMaxHypotheses = 1 << 20;

struct RelPair {
  double ka[7], kb[7];   // Camera::k of a's and b's camera
  int32_t a, b;          // map frame indices
  int32_t run, pad;      // 0: fewer than kRelMinObs records (SG_REL_DID_NOT_RUN, no workgroup work)
};
static_assert(sizeof(RelPair) == 128, "read by the kernels as 14 doubles and 4 ints");

struct RelPlan {
  std::vector<int32_t> off;       // [n + 1] records of pair i: off[i] .. off[i + 1]
  std::vector<double> records;    // [4 off[n]]
  std::vector<int32_t> obs;       // [2 off[n]] observation in a, in b
  std::vector<RelPair> pairs;     // [n]
  int num_run = 0;
  int H = 0, S = 0;               // hypotheses per pair, workgroups per pair (H / kRelThreads)
  int64_t grid = 0;               // n * S workgroups
};

// Throws sg::Error(SG_EINVAL) on every argument error of sg_slam_relative_poses' contract.  n == 0 gives an empty plan.
void PlanRelPoses(const sg_map* m, const int32_t* pairs, int32_t n, const sg_relpose_options* o, RelPlan* out);

}  // namespace sg

#endif  // SG_RELPOSE_PLAN_H_
