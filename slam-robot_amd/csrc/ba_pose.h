// ba_pose.h — pose-only bundle adjustment (sg_slam_solve_frame_poses): host driver of k_pose_lm; see ba_pose.hip.
#ifndef SG_BA_POSE_H_
#define SG_BA_POSE_H_

#include <hip/hip_runtime.h>

#include "common.h"
#include "dbuf.h"
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

class PoseSolver {
 public:
  // stream: the HIP stream to run on (the Slam facade passes its solver's); nullptr: a stream of its own
  explicit PoseSolver(const sg_device_options& dev, hipStream_t stream = nullptr);
  ~PoseSolver();
  // Solves the listed frames of m against the map as it is at entry; writes the poses of the solved frames into
  // m, solved[n] and (if not null) summaries[n].  The summaries of every listed frame are also kept in
  // summaries() until the next call.
  void Solve(sg_map* m, const int32_t* frames, int32_t n, double range, bool with_frame_distance,
             const sg_solver_options& o, int32_t* solved, sg_solver_summary* summaries);
  const std::vector<sg_solver_summary>& summaries() const { return sums_; }
  // Development aid (tools/pose_bench.py): HIP-event time of the k_pose_lm launch of the calls that follow.
  void SetTiming(bool on) { timing_ = on; }
  double last_kernel_ms() const { return kernel_ms_; }

 private:
  sg_device_options dev_;
  hipStream_t stream_ = nullptr;
  bool own_stream_ = false;
  HostIo io_;
  PosePlan plan_;
  DBuf<PoseFrame> frames_;
  DBuf<int32_t> off_;
  DBuf<PoseRecord> records_;
  DBuf<PoseOut> out_;
  std::vector<PoseOut> out_h_;
  std::vector<sg_solver_summary> sums_;
  bool timing_ = false;
  double kernel_ms_ = 0.0;
  hipEvent_t ev_[2] = {nullptr, nullptr};
};

}  // namespace sg

#endif  // SG_BA_POSE_H_
