// ba_posegraph.h — pose-graph optimisation (sg_slam_optimize_pose_graph): host driver of k_posegraph_lm; see
// ba_posegraph.hip.
#ifndef SG_BA_POSEGRAPH_H_
#define SG_BA_POSEGRAPH_H_

#include <hip/hip_runtime.h>

#include "common.h"
#include "dbuf.h"
#include "device_stream.h"
#include "hostio.h"
#include "posegraph_plan.h"

namespace sg {

// Workgroup shape of k_posegraph_lm: four waves, the shape whose fixed-order reduction (DPP wave sums, then the four
// waves in order) the other single-workgroup solvers use.
constexpr int kPgThreads = 256;
constexpr int kPgWaves = kPgThreads / 64;

class PoseGraphSolver {
 public:
  // stream: the HIP stream to run on (the Slam facade passes its solver's); nullptr: a stream of its own
  explicit PoseGraphSolver(const sg_device_options& dev, hipStream_t stream = nullptr) : stream_(dev, stream) {}
  // Solves the plan's graphs that run (one upload, one launch, one download), then writes the map, status[n],
  // log_scale (may be null) and summaries (may be null).  The summaries of every graph are also kept in summaries()
  // until the next call.
  void Solve(sg_map* m, const PgPlan& plan, const sg_posegraph_options& po, const sg_solver_options& o,
             int32_t* status, double* log_scale, sg_solver_summary* summaries);
  const std::vector<sg_solver_summary>& summaries() const { return sums_; }
  // Development aid (tools/posegraph_bench.py): HIP-event time of the k_posegraph_lm launch of the calls that follow.
  void SetTiming(bool on) { timer_.Enable(on); }
  double last_kernel_ms() const { return timer_.last_ms(); }

 private:
  DeviceStream stream_;
  HostIo io_;
  DBuf<PgGraph> graphs_;
  DBuf<int32_t> node_col_, col_node_, edge_ab_, colptr_, blk_row_, blk_col_, asm_ptr_, asm_items_, gasm_ptr_,
      gasm_items_, upd_ptr_, upd_;
  DBuf<double> edge_meas_, edge_w_, x0_, x1_, xout_, L_, rec0_, rec1_, vec_;
  DBuf<PgOut> out_;
  std::vector<PgOut> out_h_;
  std::vector<double> x_h_;
  std::vector<sg_solver_summary> sums_;
  KernelTimer timer_;
};

// sums_[g] from a graph's PgOut (shared with the CPU path of capi.cpp).
void PgSummarize(const PgOut& r, sg_solver_summary* su);

}  // namespace sg

#endif  // SG_BA_POSEGRAPH_H_
