// ba_align.h — alignment of matched landmarks (sg_slam_align_points): host driver of k_align_ransac and
// k_align_select; see ba_align.hip.
#ifndef SG_BA_ALIGN_H_
#define SG_BA_ALIGN_H_

#include <hip/hip_runtime.h>

#include "align_plan.h"
#include "common.h"
#include "dbuf.h"
#include "device_stream.h"
#include "hostio.h"

namespace sg {

// Records of a group held in LDS, six arrays (48 KiB); the records beyond are read from global memory.
constexpr int kAlignStage = 1024;

// What k_align_ransac writes per workgroup (one slice of kAlignThreads hypotheses of one group): the slice's best
// transform in loc_before's order (ba_pose.h), or h = -1 when no hypothesis of the slice gave one.
struct AlignCandidate {
  double cost, sumsq;   // sumsq: the inliers' e^2 summed in record order; cost: (N - inliers) tau^2 + sumsq
  double s, q[4], t[3];
  int32_t h, inliers;
  int32_t models, pad;  // hypotheses of the slice that gave a model
};
static_assert(sizeof(AlignCandidate) == 96, "written by k_align_ransac as 10 doubles and 4 ints");

// What k_align_select writes per group.
struct AlignOut {
  double cost, sumsq, ransac_cost, gap;
  double s, q[4], t[3];
  int32_t status, num_records, inliers, refined;
  int32_t h, models, sample[3], pad;
};
static_assert(sizeof(AlignOut) == 136, "written by k_align_select as 12 doubles and 10 ints");

class AlignSolver {
 public:
  explicit AlignSolver(const sg_device_options& dev, hipStream_t stream = nullptr) : stream_(dev, stream) {}
  // plan: PlanAlign's result for the call, made by the caller before the device is touched; num_corr: the
  // correspondences of the call (group_offset[n]).  One upload, two launches, one download.  results and corr_inlier
  // may be null.  The map is not an argument: everything the kernels read is in the plan.
  void Solve(const AlignPlan& plan, int32_t n, int32_t num_corr, const sg_align_options& o, int32_t* solved,
             sg_align_result* results, int32_t* corr_inlier);
  // Development aid (tools/align_bench.py): HIP-event time of the two launches of the calls that follow.
  void SetTiming(bool on) { timer_.Enable(on); }
  double last_kernel_ms() const { return timer_.last_ms(); }

 private:
  DeviceStream stream_;
  HostIo io_;
  DBuf<AlignGroup> groups_;
  DBuf<int32_t> off_;
  DBuf<double> records_;
  DBuf<AlignCandidate> cand_;
  DBuf<AlignOut> out_;
  DBuf<int32_t> flags_;
  std::vector<AlignOut> out_h_;
  std::vector<int32_t> flags_h_;
  KernelTimer timer_;
};

}  // namespace sg

#endif  // SG_BA_ALIGN_H_
