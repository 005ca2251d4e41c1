// ba_pose.h — pose-only bundle adjustment (sg_slam_solve_frame_poses): host driver of k_pose_lm; see ba_pose.hip.
#ifndef SG_BA_POSE_H_
#define SG_BA_POSE_H_

#include <hip/hip_runtime.h>

#include "common.h"
#include "dbuf.h"
#include "device_stream.h"
#include "hostio.h"
#include "pose_plan.h"

namespace sg {

// What k_pose_lm writes per requested frame: the solved pose and the minimizer's summary fields.
struct PoseOut {
  double q[4], t[3];
  double initial_cost, final_cost, fixed_cost, radius;
  int32_t num_iterations, n_succ, n_unsucc, n_invalid;
  int32_t termination, ok, lm_iters;
  int32_t finished;   // 1: the LM loop ended by a termination test; 0: it ran into the iteration bound (a defect)
};
static_assert(sizeof(PoseOut) == 120, "written by k_pose_lm as 11 doubles and 8 ints");

// Workgroup shape shared by k_pose_lm (ba_pose.hip) and k_pose_ransac / k_pose_select (ba_localize.hip).
constexpr int kPoseThreads = 256;
constexpr int kPoseWaves = kPoseThreads / 64;
// Records of a frame held in LDS for the whole solve, element by element (six arrays, so a wave's lanes read
// consecutive doubles): 48 KiB.  The records beyond are re-read from global memory in every sweep.
constexpr int kPoseStage = 1024;

// sg_slam_localize_frames rounds max_hypotheses up to a multiple of kPoseThreads; anything above this counts as this.
constexpr int kLocalizeMaxHypotheses = 1 << 20;

// What k_pose_ransac writes per workgroup (one slice of kPoseThreads hypotheses of one frame): the slice's best
// pose in the order of loc_before (ba_localize.hip), or h = -1 when no hypothesis of the slice gave a pose.
struct LocCandidate {
  double cost, sumsq;   // sumsq: the inliers' e^2 summed in record order; cost: (N - inliers) tau^2 + sumsq
  double q[4], t[3];
  int32_t h, root;      // hypothesis, index of the quartic's root
  int32_t inliers;      // records with e^2 <= tau^2
  int32_t models;       // hypotheses of the slice that gave at least one pose
};
static_assert(sizeof(LocCandidate) == 88, "written by k_pose_ransac as 9 doubles and 4 ints");

// What k_pose_select writes per listed frame: the figures at one pose (the RANSAC winner, or k_pose_lm's result).
struct LocOut {
  double cost, sumsq;   // MSAC cost (num_obs - inliers) tau^2 + sumsq; sum of e^2 over the inliers
  double q[4], t[3];
  int32_t status, num_obs, inliers;
  int32_t h, root, sample[3];   // the winner's hypothesis, root index and record indices (-1 without a model)
  int32_t models, pad;
};
static_assert(sizeof(LocOut) == 112, "written by k_pose_select as 9 doubles and 10 ints");

// The order of the poses of one frame: the MSAC cost T tau^2 + s as a double (T the truncated records, s the sum of
// e^2 over the inliers); then, among equal doubles, more inliers, then the smaller s; then the smaller h, then the
// smaller root index.  The two middle keys matter on clean data with outliers present, where every all-inlier
// sample's s (1e-20 px^2) vanishes in the rounding of T tau^2 + s and the rounded costs tie; they keep the most
// accurate of those poses instead of the first.  h = -1 marks "no pose" and is after everything.
struct LocKey {
  double cost, s;
  int inl, h, root;
};
__device__ __forceinline__ bool loc_before(const LocKey& a, const LocKey& b) {
  if (a.h < 0) return false;
  if (b.h < 0) return true;
  if (a.cost != b.cost) return a.cost < b.cost;
  if (a.inl != b.inl) return a.inl > b.inl;
  if (a.s != b.s) return a.s < b.s;
  if (a.h != b.h) return a.h < b.h;
  return a.root < b.root;
}

class PoseSolver {
 public:
  // stream: the HIP stream to run on (the Slam facade passes its solver's); nullptr: a stream of its own
  explicit PoseSolver(const sg_device_options& dev, hipStream_t stream = nullptr) : stream_(dev, stream) {}
  // Solves the listed frames of m against the map as it is at entry; writes the poses of the solved frames into
  // m, solved[n] and (if not null) summaries[n].  The summaries of every listed frame are also kept in
  // summaries() until the next call.
  void Solve(sg_map* m, const int32_t* frames, int32_t n, double range, bool with_frame_distance,
             const sg_solver_options& o, int32_t* solved, sg_solver_summary* summaries);
  const std::vector<sg_solver_summary>& summaries() const { return sums_; }
  // sg_slam_localize_frames (ba_localize.hip): k_pose_ransac and k_pose_select on the listed frames and, with
  // lo.refine, k_pose_lm from the winners and k_pose_select once more on its poses, all on the one stream (one
  // upload, two to four launches, one download).  The entry poses are not read.  results, obs_inlier
  // ([m->num_obs]) and summaries may be null; the polish's summaries are also kept in summaries().
  void Localize(sg_map* m, const int32_t* frames, int32_t n, const sg_localize_options& lo,
                const sg_solver_options& o, int32_t* solved, sg_localize_result* results, int32_t* obs_inlier,
                sg_solver_summary* summaries);
  // Development aid (tools/pose_bench.py, tools/localize_bench.py): HIP-event time of the k_pose_lm launch of the
  // calls that follow; after Localize, of its two to four launches.
  void SetTiming(bool on) { timer_.Enable(on); }
  double last_kernel_ms() const { return timer_.last_ms(); }

 private:
  // The pieces Solve and Localize share.  LaunchLm: k_pose_lm on the n uploaded frames (frames_, off_, records_;
  // out_ sized for n), on stream_.  Summarize: sums_[i] from out_h_[i] (SG_EDEVICE when the loop did not finish).
  void LaunchLm(int32_t n, double range, const sg_solver_options& o);
  void Summarize(int i);

  DeviceStream stream_;
  HostIo io_;
  PosePlan plan_;
  DBuf<PoseFrame> frames_;
  DBuf<int32_t> off_;
  DBuf<PoseRecord> records_;
  DBuf<PoseOut> out_;
  std::vector<PoseOut> out_h_;
  std::vector<sg_solver_summary> sums_;
  // Localize's
  DBuf<int32_t> frame_index_;
  DBuf<LocCandidate> cand_;
  DBuf<LocOut> loc_d_[2];        // at the RANSAC winner | at the polish's pose
  DBuf<int32_t> flags_d_[2];     // per record, the same two
  std::vector<LocOut> loc_h_[2];
  std::vector<int32_t> flags_h_[2];
  KernelTimer timer_;
};

}  // namespace sg

#endif  // SG_BA_POSE_H_
