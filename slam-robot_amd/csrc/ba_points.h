// ba_points.h — structure-only bundle adjustment (sg_slam_solve_points): host driver of k_point_lm; see
// ba_points.hip.
#ifndef SG_BA_POINTS_H_
#define SG_BA_POINTS_H_

#include <hip/hip_runtime.h>

#include "common.h"
#include "dbuf.h"
#include "hostio.h"
#include "points_plan.h"

namespace sg {

// What k_point_lm writes per listed point that ran: the solved location and the minimizer's summary fields.
struct PointOut {
  double X[4];
  double initial_cost, final_cost, radius;
  int32_t num_iterations, n_succ, n_unsucc, n_invalid;
  int32_t termination, ok, lm_iters;
  int32_t finished;   // 1: the LM loop ended by a termination test; 0: it ran into the iteration bound (a defect)
};
static_assert(sizeof(PointOut) == 88, "written by k_point_lm as 7 doubles and 8 ints");

class PointSolver {
 public:
  // stream: the HIP stream to run on (the Slam facade passes its solver's); nullptr: a stream of its own
  explicit PointSolver(const sg_device_options& dev, hipStream_t stream = nullptr);
  ~PointSolver();
  // Solves the listed points of m against the map as it is at entry; writes the locations of the solved points
  // into m, solved[n] and (if not null) summaries[n].  The summaries of every listed point are also kept in
  // summaries() until the next call.
  void Solve(sg_map* m, const int32_t* points, int32_t n, double range, const sg_solver_options& o, int32_t* solved,
             sg_solver_summary* summaries);
  const std::vector<sg_solver_summary>& summaries() const { return sums_; }
  // Development aid (tools/points_bench.py): HIP-event time of the k_point_lm launch of the calls that follow.
  void SetTiming(bool on) { timing_ = on; }
  double last_kernel_ms() const { return kernel_ms_; }

 private:
  sg_device_options dev_;
  hipStream_t stream_ = nullptr;
  bool own_stream_ = false;
  HostIo io_;
  PointsPlan plan_;
  DBuf<int32_t> off_;
  DBuf<PointObs> obs_;
  DBuf<PointFrame> frames_;
  DBuf<double> k_;
  DBuf<PointStart> points_;
  DBuf<PointOut> out_;
  std::vector<PointOut> out_h_;
  std::vector<sg_solver_summary> sums_;
  bool timing_ = false;
  double kernel_ms_ = 0.0;
  hipEvent_t ev_[2] = {nullptr, nullptr};
};

}  // namespace sg

#endif  // SG_BA_POINTS_H_
