// ba_match.h — match by projection (sg_slam_match_by_projection): host driver of k_match_project, k_match_window
// and k_match_merge; see ba_match.hip.
#ifndef SG_BA_MATCH_H_
#define SG_BA_MATCH_H_

#include <hip/hip_runtime.h>

#include "common.h"
#include "dbuf.h"
#include "device_stream.h"
#include "hostio.h"
#include "match_plan.h"

namespace sg {

class MatchSolver {
 public:
  explicit MatchSolver(const sg_device_options& dev, hipStream_t stream = nullptr) : stream_(dev, stream) {}
  // plan: PlanMatch's result for the call (plan.launch set), made by the caller before the device is touched; the
  // keypoints and the point list are the call's own arrays.  One upload, three launches, one download.  The four
  // per-keypoint arrays [K] and projected [n] are all written, and only after the downloaded values have been checked.
  void Run(const MatchPlan& plan, const double* kp_xy, const uint64_t* kp_desc, const int32_t* points,
           const uint64_t* point_desc, const sg_match_options& o, int32_t* best_point, int32_t* best_dist,
           int32_t* second_dist, int32_t* num_candidates, int32_t* projected);
  // Development aid (tools/match_bench.py): HIP-event time of the three launches of the calls that follow.
  void SetTiming(bool on) { timer_.Enable(on); }
  double last_kernel_ms() const { return timer_.last_ms(); }

 private:
  DeviceStream stream_;
  HostIo io_;
  DBuf<MatchFrame> frames_;
  DBuf<MatchChunk> chunks_;
  DBuf<double> X_, kp_xy_;
  DBuf<uint64_t> kp_desc_, point_desc_;
  DBuf<uint32_t> excl_;
  DBuf<int32_t> points_, count_;
  DBuf<double2> surv_uv_;      // [n * np] the survivors of listed frame i at i * np ..
  DBuf<uint4> surv_desc_;      // [2 n * np]
  DBuf<int32_t> surv_pos_;     // [n * np]
  DBuf<uint4> part_;           // [slices * K] best key, second key, window size of one slice
  DBuf<int32_t> out_;          // [4 K] best_point, best_dist, second_dist, num_candidates
  KernelTimer timer_;
};

}  // namespace sg

#endif  // SG_BA_MATCH_H_
