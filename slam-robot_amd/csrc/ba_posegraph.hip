// ba_posegraph.hip — pose-graph optimisation: sg_slam_optimize_pose_graph.
//
// The problem (nodes q | t | sigma, edges with a rotation, a translation and a scale residual, optional Cauchy loss)
// is stated in include/slamgpu.h; its arithmetic is posegraph_math.h's, its plan posegraph_plan.h's.  7 (or 6)
// unknowns per free node and a sparse coupling, so a whole Levenberg-Marquardt solve of a graph of up to kPgMaxNodes
// nodes fits in one workgroup: k_posegraph_lm runs one workgroup per graph and the entire LM loop inside one launch,
// with no hand-off between workgroups.  The minimizer's bookkeeping (iteration push, tolerance tests, step decision,
// radius update) is ba_lm.h's, the one copy the window solver uses; thread 0 runs it on a register copy, as in
// k_pose_lm.
//
// Per linearization: every edge's residual and Jacobian, strided over the threads and stored per edge; the gradient
// and the diagonal by the planner's gather lists; per step: Jacobi scale and damping, the assembly of the damped
// scaled matrix into L's pattern by the gather lists, the numeric block Cholesky column by column in elimination
// order (the diagonal block's factor on thread 0, the column's off-diagonal solves and its update triples spread over
// the threads), forward and back substitution, the candidate states, and the candidate's cost with its
// linearization (an accepted step's is then already there).  Every sum has a fixed order: a gather list's listed edge
// order, or the workgroup reduction (DPP wave sums, then the four waves in order), so a result is reproducible bit
// for bit and independent of the graph's position in the call.
//
// Decided without a device measurement of the alternatives, the simplest of each: node states, edge records and the
// factor live in global memory (a graph's working set stays in L2: the factor of a 200-node ring is 0.4 MB, and the
// 7 x 7 blocks of 1024 nodes would not fit in LDS beside anything else); 256 threads; the columns of the elimination
// tree run one after the other.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>

#include "ba_lm.h"
#include "ba_posegraph.h"

namespace sg {

namespace {

struct PgArgs {
  PgView v;
  PgOut* out;
  double* xout;   // [kPgState nodes] the solved states
  int32_t cap;    // LM loop bound (a defect ends as an error, not as a hang)
};

// One sweep over the graph's edges at x[slot]: thread t linearizes edges t, t + 256, ... into rec[slot]; the cost and
// the fixed cost by the fixed-order reduction (every thread gets the totals).
__device__ __forceinline__ void pg_sweep(const PgView& v, const PgGraph& G, int slot, double* red, double* cost,
                                         double* fixed_cost) {
  double c = 0.0, f = 0.0;
  for (int e = threadIdx.x; e < G.ne; e += kPgThreads) {
    bool fx;
    const double x = PgEdgeLinearize(v, G, e, slot, &fx);
    if (fx) f += x;
    else c += x;
  }
  *cost = block_sum<kPgThreads>(c, red);
  *fixed_cost = block_sum<kPgThreads>(f, red);
}

__global__ __launch_bounds__(kPgThreads) void k_posegraph_lm(PgArgs a, LmState init) {
  __shared__ double red[kPgWaves];
  __shared__ double dsh[2];   // radius
  __shared__ int ctl[8];      // done | reuse_diag | pivot ok | cur | need_lin
  const PgView& v = a.v;
  const PgGraph G = v.graphs[blockIdx.x];
  if (!G.run) return;   // (the whole workgroup: decided by the planner)
  const int tid = threadIdx.x;
  const int D = v.D, dd = D * D, nx = G.nc * D;

  double slot_cost[2] = {0.0, 0.0}, fx0;
  pg_sweep(v, G, 0, red, &slot_cost[0], &fx0);
  double xn2 = 0.0;
  for (int nd = tid; nd < G.nn; nd += kPgThreads) xn2 += PgNodeNorm2(v, G, nd, 0);
  xn2 = block_sum<kPgThreads>(xn2, red);

  // thread 0 runs the minimizer on register copies; the other threads follow it through ctl
  LmState s = init;
  double u[kUNum];
  const double c[kCNum] = {0, 0, 0, 0, 0, 0};   // no second solver stage: the Cholesky's slots stay zero
#pragma unroll
  for (int i = 0; i < kUNum; ++i) u[i] = 0.0;
  int cur = 0, lin = 1, first = 1;
  for (int it = 0; it < a.cap; ++it) {
    if (lin) {
      double gm = 0.0;
      for (int i = tid; i < nx; i += kPgThreads) {
        PgGradEntry(v, G, i, cur);
        const size_t at = 7 * (size_t)(G.col0 + i / D) + i % D;
        gm = fmax(gm, fabs(v.g[at]));
        if (first) v.scale[at] = init.jacobi ? 1.0 / (1.0 + sqrt(v.hd[at])) : 1.0;
      }
      gm = block_max<kPgThreads>(gm, red);
      if (tid == 0) {
        double xs[kXNum];
        xs[kXCost] = slot_cost[cur];
        xs[kXFail] = 0.0;
        xs[kXFixed] = fx0;
        xs[kXFixedFail] = 0.0;
        xs[kXXnorm2] = xn2;
        fin_push(s, first, slot_cost[cur], gm, xs, 0.0);
      }
    }
    if (tid == 0) {
      fin_count(s);
      ctl[0] = s.done;
      ctl[1] = s.reuse_diag;
      dsh[0] = s.radius;
    }
    __syncthreads();
    if (ctl[0]) break;
    const int reuse = ctl[1];
    const double radius = dsh[0];
    // LevenbergMarquardtStrategy::ComputeStep on the Jacobi-scaled system: (S H S + D / radius) y = S g
    for (int i = tid; i < nx; i += kPgThreads) {
      const size_t at = 7 * (size_t)(G.col0 + i / D) + i % D;
      const double sc = v.scale[at];
      if (!reuse) v.diag[at] = fmin(fmax(sc * sc * v.hd[at], init.min_diag), init.max_diag);
      v.y[at] = v.g[at] * sc;
    }
    __syncthreads();
    for (int i = tid; i < G.nb * dd; i += kPgThreads) PgAssembleEntry(v, G, i, cur, radius);
    __syncthreads();
    bool okf = true;
    for (int j = 0; j < G.nc; ++j) {
      if (tid == 0) ctl[2] = PgFactorDiag(v, G, j) ? 1 : 0;
      __syncthreads();
      if (!ctl[2]) {   // (the whole workgroup) non-positive pivot: the step is invalid
        okf = false;
        break;
      }
      const int rows = v.colptr[G.col0 + j + 1] - v.colptr[G.col0 + j] - 1;
      for (int i = tid; i < rows * D; i += kPgThreads) PgSolveOffRow(v, G, j, i);
      __syncthreads();
      const int nu = v.upd_ptr[G.col0 + j + 1] - v.upd_ptr[G.col0 + j];
      for (int i = tid; i < nu * dd; i += kPgThreads) PgUpdateEntry(v, G, j, i);
      __syncthreads();
    }
    double mdl = 0.0, step2 = 0.0, candx2 = 0.0;
    if (okf) {
      for (int j = 0; j < G.nc; ++j) {
        if (tid == 0) PgForwardDiag(v, G, j);
        __syncthreads();
        const int rows = v.colptr[G.col0 + j + 1] - v.colptr[G.col0 + j] - 1;
        for (int i = tid; i < rows * D; i += kPgThreads) PgForwardRow(v, G, j, i);
        __syncthreads();
      }
      for (int j = G.nc - 1; j >= 0; --j) {
        if (tid < D) PgBackwardGather(v, G, j, tid);
        __syncthreads();
        if (tid == 0) PgBackwardDiag(v, G, j);
        __syncthreads();
      }
      double sums[2] = {0.0, 0.0};
      for (int nd = tid; nd < G.nn; nd += kPgThreads) PgCandidateNode(v, G, nd, cur, sums);
      __syncthreads();
      for (int e = tid; e < G.ne; e += kPgThreads) mdl += PgModelEdge(v, G, e, cur);
      double fxc;
      pg_sweep(v, G, cur ^ 1, red, &slot_cost[cur ^ 1], &fxc);
      mdl = block_sum<kPgThreads>(mdl, red);
      step2 = block_sum<kPgThreads>(sums[0], red);
      candx2 = block_sum<kPgThreads>(sums[1], red);
    }
    if (tid == 0) {
      u[kULinFail] = okf ? 0.0 : 1.0;
      u[kUModel] = mdl;
      u[kUStep2] = step2;
      u[kUCandX2] = candx2;
      u[kUCandCost] = okf ? slot_cost[cur ^ 1] : 0.0;
      u[kUCandFail] = 0.0;
      decide_step(s, u, c);   // accepted: s.cur flips to the candidate's slot, whose linearization is rec[cur ^ 1]
      ctl[3] = s.cur;
      ctl[4] = s.need_lin;
    }
    __syncthreads();
    cur = ctl[3];
    lin = ctl[4];
    first = 0;
    __syncthreads();   // ctl is rewritten by the next iteration
  }
  for (int i = tid; i < kPgState * G.nn; i += kPgThreads)
    a.xout[kPgState * (size_t)G.node0 + i] = v.x[cur][kPgState * (size_t)G.node0 + i];
  if (tid == 0) {
    PgOut o;
    o.initial_cost = s.initial_cost;
    o.final_cost = s.min_pushed_cost + s.fixed_cost;
    o.fixed_cost = s.fixed_cost;
    o.radius = s.radius;
    o.num_iterations = s.pushed;
    o.n_succ = s.n_succ;
    o.n_unsucc = s.n_unsucc;
    o.n_invalid = s.n_invalid;
    o.termination = s.termination;
    o.ok = s.ok;
    o.lm_iters = s.lm_iters;
    o.finished = s.done;
    o.cur = cur;
    o.pad = 0;
    a.out[blockIdx.x] = o;
  }
}

}  // namespace

void PgSummarize(const PgOut& r, sg_solver_summary* su) {
  SG_REQUIRE(r.finished, SG_EDEVICE, "LM loop did not terminate on the device");
  su->num_iterations = r.num_iterations;
  su->num_successful_steps = r.n_succ;
  su->num_unsuccessful_steps = r.n_unsucc;
  su->num_invalid_steps = r.n_invalid;
  su->termination_type = r.termination;
  su->ok = r.ok;
  su->initial_cost = r.initial_cost;
  su->final_cost = r.final_cost;
  su->fixed_cost = r.fixed_cost;
  su->trust_region_radius = r.radius;
  su->num_lm_iterations = r.lm_iters;
  su->sync_timeouts = 0;   // nothing to time out on: no hand-off between workgroups
}

void PoseGraphSolver::Solve(sg_map* m, const PgPlan& plan, const sg_posegraph_options& po, const sg_solver_options& o,
                            int32_t* status, double* log_scale, sg_solver_summary* summaries) {
  const int n = (int)plan.graphs.size();
  sg_solver_summary none{};
  none.termination_type = SG_DID_NOT_RUN;
  sums_.assign((size_t)n, none);
  timer_.Reset();
  std::vector<int32_t> st((size_t)n);
  for (int g = 0; g < n; ++g) st[g] = plan.graphs[g].status;
  const size_t N = plan.node_col.size(), E = plan.edge_ab.size() / 2, B = plan.blk_row.size(),
               C = plan.col_node.size();
  x_h_.assign(plan.x0.begin(), plan.x0.end());
  if (plan.num_run > 0) {
    stream_.Bind();
    io_.Begin();
    io_.Up(graphs_, plan.graphs);
    io_.Up(node_col_, plan.node_col);
    io_.Up(col_node_, plan.col_node);
    io_.Up(edge_ab_, plan.edge_ab);
    io_.Up(edge_meas_, plan.edge_meas);
    io_.Up(edge_w_, plan.edge_w);
    io_.Up(colptr_, plan.colptr);
    io_.Up(blk_row_, plan.blk_row);
    io_.Up(blk_col_, plan.blk_col);
    io_.Up(asm_ptr_, plan.asm_ptr);
    io_.Up(asm_items_, plan.asm_items);
    io_.Up(gasm_ptr_, plan.gasm_ptr);
    io_.Up(gasm_items_, plan.gasm_items);
    io_.Up(upd_ptr_, plan.upd_ptr);
    io_.Up(upd_, plan.upd);
    io_.Up(x0_, plan.x0);
    x1_.Resize(std::max<size_t>(kPgState * N, 1));
    xout_.Resize(std::max<size_t>(kPgState * N, 1));
    L_.Resize(std::max<size_t>(kPgBlk * B, 1));
    rec0_.Resize(std::max<size_t>((size_t)kPgRec * E, 1));
    rec1_.Resize(std::max<size_t>((size_t)kPgRec * E, 1));
    vec_.Resize(std::max<size_t>(6 * 7 * C, 1));
    out_.Resize((size_t)n);
    io_.FlushUp(stream_.get());

    LmState s{};   // as BaSolver::Begin
    s.max_iter = o.max_num_iterations;
    s.max_invalid = o.max_num_consecutive_invalid_steps;
    s.disable_term = o.disable_termination;
    s.always_lin = o.always_linearize;
    s.jacobi = o.jacobi_scaling;
    s.ftol = o.function_tolerance;
    s.gtol = o.gradient_tolerance;
    s.ptol = o.parameter_tolerance;
    s.min_rel_dec = o.min_relative_decrease;
    s.max_radius = o.max_trust_region_radius;
    s.min_radius = o.min_trust_region_radius;
    s.min_diag = o.min_lm_diagonal;
    s.max_diag = o.max_lm_diagonal;
    s.need_lin = 1;
    s.first = 1;
    s.ok = 1;
    s.termination = SG_NO_CONVERGENCE;
    s.radius = o.initial_trust_region_radius;
    s.decrease_factor = 2.0;
    PgArgs a{};
    PgView& v = a.v;
    v.graphs = graphs_.ptr;
    v.node_col = node_col_.ptr;
    v.col_node = col_node_.ptr;
    v.edge_ab = edge_ab_.ptr;
    v.edge_meas = edge_meas_.ptr;
    v.edge_w = edge_w_.ptr;
    v.colptr = colptr_.ptr;
    v.blk_row = blk_row_.ptr;
    v.blk_col = blk_col_.ptr;
    v.asm_ptr = asm_ptr_.ptr;
    v.asm_items = asm_items_.ptr;
    v.gasm_ptr = gasm_ptr_.ptr;
    v.gasm_items = gasm_items_.ptr;
    v.upd_ptr = upd_ptr_.ptr;
    v.upd = upd_.ptr;
    v.L = L_.ptr;
    v.rec[0] = rec0_.ptr;
    v.rec[1] = rec1_.ptr;
    v.x[0] = x0_.ptr;
    v.x[1] = x1_.ptr;
    v.g = vec_.ptr;
    v.hd = vec_.ptr + 7 * C;
    v.scale = vec_.ptr + 2 * 7 * C;
    v.diag = vec_.ptr + 3 * 7 * C;
    v.y = vec_.ptr + 4 * 7 * C;
    v.delta = vec_.ptr + 5 * 7 * C;
    v.D = plan.D;
    v.fix_scale = plan.fix_scale;
    v.b = plan.b;
    v.inv_b = plan.inv_b;
    a.out = out_.ptr;
    a.xout = xout_.ptr;
    // the bound of BaSolver::Solve's host loop: every iteration, rejected and invalid steps included
    const long long cap =
        (long long)std::max(o.max_num_iterations, 0) * (std::max(o.max_num_consecutive_invalid_steps, 0) + 2) + 16;
    a.cap = (int32_t)std::min<long long>(cap, INT_MAX);
    timer_.Start(stream_.get());
    hipLaunchKernelGGL(k_posegraph_lm, dim3((unsigned)n), dim3(kPgThreads), 0, stream_.get(), a, s);
    SG_HIP_CHECK(hipGetLastError());
    timer_.Stop(stream_.get());
    out_h_.resize((size_t)n);
    x_h_.resize(kPgState * N);
    io_.Down(out_h_.data(), out_.ptr, (size_t)n * sizeof(PgOut));
    io_.Down(x_h_.data(), xout_.ptr, kPgState * N * sizeof(double));
    io_.FinishDown(stream_.get());
    timer_.Read();
    for (int g = 0; g < n; ++g) {
      if (!plan.graphs[g].run) continue;
      PgSummarize(out_h_[g], &sums_[g]);
      if (!sums_[g].ok) st[g] = SG_PG_FAILED;
    }
  }
  // write-back only after every graph's result has been checked: a failed call changes nothing
  PgWriteBack(m, plan, st.data(), x_h_.data(), po.move_points, log_scale);
  for (int g = 0; g < n; ++g) status[g] = st[g];
  if (summaries)
    for (int g = 0; g < n; ++g) summaries[g] = sums_[g];
}

}  // namespace sg
