// posegraph_plan.h — the host-only planner of sg_slam_optimize_pose_graph (ba_posegraph.hip): from an sg_map, the
// graphs' node and edge lists and the options, everything k_posegraph_lm reads.  A pure function of its arguments (no
// HIP, no environment, no state, no I/O), so a CPU test recomputes it by brute force
// (tests/native/posegraph_plan_check.cpp).
//
// Per graph:
//   - the component and anchor test: no free node, or no edge at a free node: SG_PG_DID_NOT_RUN; a connected component
//     (over all listed edges) with a free node and no fixed node: SG_PG_NO_ANCHOR;
//   - the elimination order: free nodes become columns by greedy minimum degree on the block graph of J^T J (an exact
//     fill simulation), ties to the lower list position;
//   - the symbolic factorisation: L's block pattern, lower, column-major, a diagonal block first in every column and
//     the rows below it ascending, blocks numbered in that order;
//   - the assembly lists: for every block of L and every gradient segment the (edge, sub-block) contributions in
//     listed edge order (a gather with a fixed summation order, no atomics);
//   - the update lists: per column j the triples (L_ij, L_kj) -> block (i, k), i >= k > j; a target appears at most
//     once per column.
// The CPU executor (PgCpuFactorSolve) runs the numeric factorisation and both triangular solves by following the plan
// with posegraph_math.h's per-entry functions, the ones the kernel strides over its threads; PgCpuSolve wraps it in
// the same Levenberg-Marquardt loop (Ceres 1.8, as ba_lm.h restates it) for the checks and tools/posegraph_bench.py.
#ifndef SG_POSEGRAPH_PLAN_H_
#define SG_POSEGRAPH_PLAN_H_

#include <cstdint>
#include <vector>

#include "posegraph_math.h"
#include "slamgpu.h"

namespace sg {

// Size caps (SG_EINVAL above them).  They bound a call's device workspace: L 49 doubles per block (50 MiB), two edge
// linearizations of 105 doubles per edge (53 MiB), the update triples (48 MiB), the lists and states (a few MiB).
constexpr int kPgMaxNodes = 1024;            // nodes per graph
constexpr int kPgMaxEdges = 8192;            // edges per graph
constexpr int kPgMaxCallNodes = 1 << 16;     // nodes per call
constexpr int kPgMaxCallEdges = 1 << 15;     // edges per call
constexpr int kPgMaxCallBlocks = 1 << 17;    // blocks of L per call
constexpr int kPgMaxCallUpdates = 1 << 22;   // update triples per call

struct PgPlan {
  std::vector<PgGraph> graphs;
  std::vector<int32_t> node_col, col_node, edge_ab;
  std::vector<double> edge_meas, edge_w;
  std::vector<int32_t> colptr, blk_row, blk_col, asm_ptr, asm_items, gasm_ptr, gasm_items, upd_ptr, upd;
  std::vector<double> x0;            // [kPgState nodes] the map's poses at entry, sigma = 0
  std::vector<int32_t> node_frame;   // [nodes] map frame index
  int num_run = 0;
  int D = 7, fix_scale = 0;
  double b = 0.0, inv_b = 0.0;
  // A view on host storage of the caller's: ws must hold PgWorkspaceDoubles() doubles.
  PgView View(double* ws) const;
  size_t WorkspaceDoubles() const;
};

// Throws sg::Error(SG_EINVAL) on every argument error of sg_slam_optimize_pose_graph's contract that concerns the map,
// the lists and the options.  n == 0 gives an empty plan (the lists are then not read and may be null).
void PlanPoseGraph(const sg_map* m, const int32_t* node_frame, const int32_t* node_fixed, const int32_t* node_offset,
                   const int32_t* edge_ab, const double* edge_meas, const double* edge_weight,
                   const int32_t* edge_offset, int32_t n, const sg_posegraph_options* o, PgPlan* out);

// Graph g's linear solve on the host: L (assembled in v.L) is factored in place and v.y (the scaled gradient) is
// replaced by the solution of L L^T y = gs.  False on a non-positive pivot.
bool PgCpuFactorSolve(const PgView& v, const PgGraph& G);

// What one graph's solve leaves (the device writes the same record, ba_posegraph.h).
struct PgOut {
  double initial_cost, final_cost, fixed_cost, radius;
  int32_t num_iterations, n_succ, n_unsucc, n_invalid;
  int32_t termination, ok, lm_iters;
  int32_t finished;   // 1: the LM loop ended by a termination test; 0: it ran into the iteration bound (a defect)
  int32_t cur, pad;   // the slot of x that holds the result
};
static_assert(sizeof(PgOut) == 72, "written by k_posegraph_lm as 4 doubles and 10 ints");

// The whole LM of graph g on the host, on the plan's lists and a workspace view; the result is x[out->cur].
void PgCpuSolve(const PgView& v, const PgGraph& G, const sg_solver_options& o, PgOut* out);

// The host-only write-back shared by the device driver and the CPU path: poses of the SG_PG_OK graphs into the map
// (q normalised with w >= 0), log_scale per listed node, and with move_points the points' move with their anchors.
// xres: [kPgState nodes] the solved states.
void PgWriteBack(sg_map* m, const PgPlan& plan, const int32_t* status, const double* xres, int move_points,
                 double* log_scale);

}  // namespace sg

#endif  // SG_POSEGRAPH_PLAN_H_
