// pose_plan.h — the host-only planner of sg_slam_solve_frame_poses (pose-only bundle adjustment, ba_pose.hip):
// from an sg_map and a list of frames, everything k_pose_lm reads.  A pure function of its arguments (no HIP, no
// environment, no state, no I/O), so a CPU test can recompute it by brute force (tests/native/pose_plan_check.cpp).
//
// Per requested frame: its usable observations (not disabled, point slam-usable: the filter of
// sg_problem_from_map_frames, slam.cpp:280-283) in map order, as packed 48-byte records with the point gathered
// on the host, so the upload is proportional to the observations used and the kernel's reads are contiguous; its
// pose, its camera's intrinsics, the translation of its previous frame and whether the FrameDistance block is
// present.  A frame with fewer than kPoseMinObs usable observations is not solved (three points are the fewest
// that determine six degrees of freedom): decided here, before anything is launched.
#ifndef SG_POSE_PLAN_H_
#define SG_POSE_PLAN_H_

#include <cstdint>
#include <vector>

#include "slamgpu.h"

namespace sg {

constexpr int kPoseMinObs = 3;
// sg_slam_localize_frames' run rule: a minimal P3P sample takes three records and leaves up to four poses; the
// fourth record is the fewest that can tell them apart.
constexpr int kLocalizeMinObs = 4;

// One usable observation: the observed pixel and its point's homogeneous location.
struct PoseRecord {
  double u, v;
  double X[4];
};
static_assert(sizeof(PoseRecord) == 48, "k_pose_lm reads records as 6 doubles");

// One requested frame.
struct PoseFrame {
  double q[4], t[3];   // the pose at entry (Eigen [x,y,z,w] memory)
  double k[7];         // Camera::k of the frame's camera
  double tprev[3];     // translation of Frame::previous() (zero without one)
  int32_t has_dist;    // FrameDistance(150) + CauchyLoss(15) to tprev is part of the problem
  int32_t run;         // 0: fewer than kPoseMinObs usable observations (SG_DID_NOT_RUN, no workgroup work)
};
static_assert(sizeof(PoseFrame) == 144, "k_pose_lm reads frames as 17 doubles and 2 ints");

struct PosePlan {
  std::vector<int32_t> off;         // [n + 1] records of requested frame i: off[i] .. off[i + 1]
  std::vector<PoseRecord> records;  // [off[n]]
  std::vector<PoseFrame> frames;    // [n]
  std::vector<int32_t> obs;         // [off[n]] each record's observation index in the map (with_obs_index only)
  int num_run = 0;                  // frames with run = 1
};

// Throws sg::Error(SG_EINVAL) on a frame index out of range or listed twice and on a map whose indices are out
// of range.  n >= 0; frames may be null when n == 0.  min_obs: the fewest records a frame needs for run = 1.
void PlanPoses(const sg_map& m, const int32_t* frames, int32_t n, bool with_frame_distance, PosePlan* out,
               int min_obs = kPoseMinObs, bool with_obs_index = false);

}  // namespace sg

#endif  // SG_POSE_PLAN_H_
