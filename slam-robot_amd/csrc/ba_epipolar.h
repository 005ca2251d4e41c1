// ba_epipolar.h — match along epipolar lines (sg_slam_match_epipolar): host driver of k_epi_prep, k_epi_window and
// k_epi_merge; see ba_epipolar.hip.
#ifndef SG_BA_EPIPOLAR_H_
#define SG_BA_EPIPOLAR_H_

#include <hip/hip_runtime.h>

#include "common.h"
#include "dbuf.h"
#include "device_stream.h"
#include "epipolar_plan.h"
#include "hostio.h"

namespace sg {

class EpipolarSolver {
 public:
  explicit EpipolarSolver(const sg_device_options& dev, hipStream_t stream = nullptr) : stream_(dev, stream) {}
  // plan: PlanEpipolar's result for the call (plan.launch set), made by the caller before the device is touched; the
  // keypoint arrays are the call's own.  One upload, three launches, one download.  The four per-keypoint arrays [KA]
  // are all written (the empty answers for the pairs that are not live), and only after the downloaded values have
  // been checked.
  void Run(const EpipolarPlan& plan, const int32_t* a_offset, const double* a_xy, const uint64_t* a_desc,
           const int32_t* a_level, const int32_t* b_offset, const double* b_xy, const uint64_t* b_desc,
           const int32_t* b_level, const sg_epipolar_options& o, int32_t* best_kp, int32_t* best_dist,
           int32_t* second_dist, int32_t* num_candidates);
  // Development aid (tools/epipolar_bench.py): HIP-event time of the three launches of the calls that follow.
  void SetTiming(bool on) { timer_.Enable(on); }
  double last_kernel_ms() const { return timer_.last_ms(); }

 private:
  DeviceStream stream_;
  HostIo io_;
  DBuf<EpiPair> pairs_;
  DBuf<EpiPrepItem> prep_;
  DBuf<EpiItem> items_;
  DBuf<EpiChunkItem> chunks_;
  DBuf<double> a_xy_, b_xy_;
  DBuf<uint64_t> a_desc_, b_desc_;
  DBuf<int32_t> a_level_, b_level_;
  DBuf<EpiA> a_rec_;           // [KA]
  DBuf<EpiB> b_rec_;           // [KB]
  DBuf<uint4> part_;           // [plan.partials] best key, second key, candidates of one slice
  DBuf<int32_t> out_;          // [4 KA] best_kp, best_dist, second_dist, num_candidates
  KernelTimer timer_;
};

}  // namespace sg

#endif  // SG_BA_EPIPOLAR_H_
