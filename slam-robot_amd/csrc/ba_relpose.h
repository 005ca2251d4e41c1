// ba_relpose.h — relative pose of frame pairs (sg_slam_relative_poses): host driver of k_relpose_ransac and
// k_relpose_select; see ba_relpose.hip.
#ifndef SG_BA_RELPOSE_H_
#define SG_BA_RELPOSE_H_

#include <hip/hip_runtime.h>

#include "common.h"
#include "dbuf.h"
#include "device_stream.h"
#include "hostio.h"
#include "relpose_plan.h"

namespace sg {

// Records of a pair held in LDS after undistortion, four arrays (32 KiB); the records beyond are read from global
// memory and undistorted at every read.
constexpr int kRelStage = 1024;

// What k_relpose_ransac writes per workgroup (one slice of kRelThreads hypotheses of one pair): the slice's best
// model in loc_before's order (ba_pose.h), or h = -1 when no hypothesis of the slice gave one.
struct RelCandidate {
  double cost, sumsq;   // sumsq: the inliers' e^2 summed in record order; cost: (N - inliers) tau^2 + sumsq
  double E[9];
  int32_t h, inliers;
  int32_t models, pad;  // hypotheses of the slice that gave a model
};
static_assert(sizeof(RelCandidate) == 104, "written by k_relpose_ransac as 11 doubles and 4 ints");

// What k_relpose_select writes per pair.
struct RelOut {
  double cost, sumsq, ransac_cost;
  double q[4], t[3], E[9];
  int32_t status, num_obs, inliers, front, parallax, refined;
  int32_t h, models, sample[8];
};
static_assert(sizeof(RelOut) == 216, "written by k_relpose_select as 19 doubles and 16 ints");

class RelPoseSolver {
 public:
  explicit RelPoseSolver(const sg_device_options& dev, hipStream_t stream = nullptr) : stream_(dev, stream) {}
  // plan: PlanRelPoses' result for (m, pairs, n, o), made by the caller before the device is touched.  One upload,
  // two launches, one download; then the write-back of step 8.  results, rec_offset, rec_inlier, rec_obs may be null.
  void Solve(sg_map* m, const RelPlan& plan, int32_t n, const sg_relpose_options& o, int32_t* solved,
             sg_relpose_result* results, int32_t* rec_offset, int32_t* rec_inlier, int32_t* rec_obs);
  // Development aid (tools/relpose_bench.py): HIP-event time of the two launches of the calls that follow.
  void SetTiming(bool on) { timer_.Enable(on); }
  double last_kernel_ms() const { return timer_.last_ms(); }

 private:
  DeviceStream stream_;
  HostIo io_;
  DBuf<RelPair> pairs_;
  DBuf<int32_t> off_;
  DBuf<double> records_;
  DBuf<RelCandidate> cand_;
  DBuf<RelOut> out_;
  DBuf<int32_t> flags_;
  std::vector<RelOut> out_h_;
  std::vector<int32_t> flags_h_;
  KernelTimer timer_;
};

}  // namespace sg

#endif  // SG_BA_RELPOSE_H_
