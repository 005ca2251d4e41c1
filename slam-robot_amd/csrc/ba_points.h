// ba_points.h — structure-only bundle adjustment (sg_slam_solve_points): host driver of k_point_lm; see
// ba_points.hip.  The same driver runs sg_slam_triangulate_points (k_point_triangulate, ba_triangulate.hip), whose
// polish is k_point_lm on the same upload.
#ifndef SG_BA_POINTS_H_
#define SG_BA_POINTS_H_

#include <hip/hip_runtime.h>

#include "common.h"
#include "dbuf.h"
#include "device_stream.h"
#include "hostio.h"
#include "points_plan.h"

namespace sg {

constexpr int kPointThreads = 256;
// Lanes per point.  8 sits at the mean track length of the SLAM maps (7.6 observations per point at C2, 10 at
// C5), and a wave waits for the slowest of 64 / 8 = 8 points, not of 64.  sum8_dpp is written for this size.
constexpr int kPointGroup = 8;
constexpr int kPointsPerBlock = kPointThreads / kPointGroup;
static_assert(kPointGroup == 8, "sum8_dpp: quad perms and the half-row mirror span 8 lanes");

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
  explicit PointSolver(const sg_device_options& dev, hipStream_t stream = nullptr) : stream_(dev, stream) {}
  // Solves the listed points of m against the map as it is at entry; writes the locations of the solved points
  // into m, solved[n] and (if not null) summaries[n].  The summaries of every listed point are also kept in
  // summaries() until the next call.
  void Solve(sg_map* m, const int32_t* points, int32_t n, double range, const sg_solver_options& o, int32_t* solved,
             sg_solver_summary* summaries);
  const std::vector<sg_solver_summary>& summaries() const { return sums_; }
  // sg_slam_triangulate_points (ba_triangulate.hip): k_point_triangulate on the listed points and, with
  // t.refine, k_point_lm from the triangulated locations on the same stream (one upload, two launches, one
  // download).  Writes the locations of the SG_TRI_OK points into m, solved[n] and (if not null) results[n] and
  // summaries[n]; summaries() holds the polish's summaries (SG_DID_NOT_RUN where it did not run).
  void Triangulate(sg_map* m, const int32_t* points, int32_t n, const sg_triangulate_options& t,
                   const sg_solver_options& o, int32_t* solved, sg_triangulate_result* results,
                   sg_solver_summary* summaries);
  const std::vector<sg_triangulate_result>& triangulation_results() const { return tri_; }
  // Development aid (tools/points_bench.py, tools/triangulate_bench.py): HIP-event time of the kernel launches of
  // the calls that follow.
  void SetTiming(bool on) { timer_.Enable(on); }
  double last_kernel_ms() const { return timer_.last_ms(); }

 private:
  // The pieces Solve and Triangulate share.  Upload: plan_ to the device (out_ sized for n points).  LaunchLm:
  // k_point_lm on the uploaded plan.  Summarize: out_h_[i] into sums_[i].
  void Upload(int32_t n);
  void LaunchLm(int32_t n, double range, const sg_solver_options& o);
  void Summarize(int32_t i);

  DeviceStream stream_;
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
  DBuf<sg_triangulate_result> tri_d_;
  std::vector<sg_triangulate_result> tri_, tri_h_;
  KernelTimer timer_;
};

}  // namespace sg

#endif  // SG_BA_POINTS_H_
