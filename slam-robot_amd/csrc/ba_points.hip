// ba_points.hip — structure-only bundle adjustment: sg_slam_solve_points.
//
// For each listed point, the Ceres problem in which only that point is free: one ReprojectionError +
// CauchyLoss(range) (slam.cpp:60-84, 285-294) per enabled observation of the point, from whatever frame, the
// homogeneous block X[4] free without a parameterization (as slam.cpp leaves it), every frame and the intrinsics
// constant, no FrameDistance.  Four unknowns per point and no coupling between points, so there is no camera
// system, no Schur complement and no band Cholesky: k_point_lm gives each point a group of kPointGroup consecutive
// lanes and runs its whole Levenberg-Marquardt loop inside one launch, in registers, with no hand-off between
// workgroups and no LDS.  The minimizer's bookkeeping (iteration push, tolerance tests, step decision, radius
// update) is ba_lm.h's, the one copy the window solver and k_pose_lm use.
//
// Per LM iteration one sweep over the point's observation records: lane j of the group linearizes records j,
// j + 8, ... at the candidate x + delta, the 16 sums are combined by a fixed DPP butterfly that leaves identical
// bits in all 8 lanes, and every lane then runs the same 4x4 solve and bookkeeping redundantly, so nothing is
// broadcast and nothing waits on a barrier.  The candidate is linearized when it is evaluated, so an accepted
// step's normal equations are already there (a rejected step's are dropped).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>

#include "ba_lm.h"
#include "ba_points.h"

namespace sg {

namespace {

// A linearization's sums: the 10 upper entries of J^T J (u4 order) | J^T r (4) | cost | behind-camera count
constexpr int kPtNV = 16;
constexpr int kPG = 10, kPCost = 14, kPFail = 15;

struct PointArgs {
  const int32_t* off;
  const PointObs* obs;
  const PointFrame* frames;
  const double* k;
  const PointStart* points;
  PointOut* out;
  double b, inv_b;   // CauchyLoss(range): b = range^2
  int32_t n;
  int32_t cap;       // LM loop bound (a defect ends as an error, not as a hang)
};

// One sweep over a point's records at location X: this lane's records (lane, lane + 8, ... of cnt, in that
// order), then the group sum.  Every lane of the wave calls it (idle lanes with cnt = 0), so the DPP butterfly
// runs under a full EXEC mask; v[kPtNV] holds the totals in every lane of the group, bit for bit the same
// whatever else the call lists and wherever the group sits in the grid.  The records, the frame table and the
// cameras are read from global memory in every sweep (small and cache-resident; keeping a lane's first record in
// registers instead was measured and is slower).
__device__ __forceinline__ void point_linearize(const PointArgs& a, const PointObs* R, int cnt, int lane,
                                                const double* X, double* v) {
#pragma unroll
  for (int j = 0; j < kPtNV; ++j) v[j] = 0.0;
  for (int i = lane; i < cnt; i += kPointGroup) {
    const PointObs ob = R[i];
    const PointFrame& fr = a.frames[ob.frame];
    const double* kp = a.k + 7 * (size_t)fr.camera;
    double q[4], t[3], k[7];
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = fr.q[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = fr.t[c];
#pragma unroll
    for (int c = 0; c < 7; ++c) k[c] = kp[c];
    const double pt[2] = {ob.u, ob.v};
    double r[2], Jc[12], Jp[8], c;
    if (!LinearizeObservation(q, t, k, X, pt, a.b, a.inv_b, r, Jc, Jp, &c)) {
      v[kPFail] += 1.0;
      continue;
    }
    int e = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
#pragma unroll
      for (int p2 = p; p2 < 4; ++p2) v[e++] += Jp[p] * Jp[p2] + Jp[4 + p] * Jp[4 + p2];
      v[kPG + p] += Jp[p] * r[0] + Jp[4 + p] * r[1];
    }
    v[kPCost] += c;
  }
#pragma unroll
  for (int j = 0; j < kPtNV; ++j) v[j] = sum8_dpp(v[j]);
}

__device__ __forceinline__ double point_norm2(const double* x) {
  return (x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]);
}

// Eight lanes per listed point; the whole Ceres 1.8 LM loop (TrustRegionMinimizer + LevenbergMarquardtStrategy as
// ba_lm.h restates them) of its 4-unknown problem.  The loop's exit is wave-uniform: a finished (or idle) group
// waits behind LmState::done until no lane of its wave is active.
__global__ __launch_bounds__(kPointThreads) void k_point_lm(PointArgs a, LmState init) {
  const int gid = blockIdx.x * kPointThreads + threadIdx.x;
  const int pi = gid / kPointGroup, lane = gid % kPointGroup;
  const bool listed = pi < a.n;
  const bool run = listed && a.points[listed ? pi : 0].run != 0;
  const int o0 = run ? a.off[pi] : 0, cnt = run ? a.off[pi + 1] - o0 : 0;
  const PointObs* R = a.obs + o0;
  double x[4] = {0, 0, 0, 0};
  if (run)
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = a.points[pi].X[i];

  double S[kPtNV];   // the linearization at x
  point_linearize(a, R, cnt, lane, x, S);

  LmState s = init;
  if (!run) s.done = 1;   // (padding lanes and DID_NOT_RUN points: idle, nothing written)
  double scale[4] = {1, 1, 1, 1}, diag[4] = {0, 0, 0, 0};
  double u[kUNum];
  const double c[kCNum] = {0, 0, 0, 0, 0, 0};   // no second solver stage: the Cholesky's slots stay zero
#pragma unroll
  for (int i = 0; i < kUNum; ++i) u[i] = 0.0;
  for (int it = 0; it < a.cap; ++it) {
    double xc[4] = {0, 0, 0, 0};
    bool eval = false;
    if (!s.done) {
      if (s.need_lin) {
        double gmax = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) gmax = fmax(gmax, fabs(S[kPG + i]));
        const bool first = s.first;
        if (first && s.jacobi)
#pragma unroll
          for (int i = 0; i < 4; ++i) scale[i] = 1.0 / (1.0 + sqrt(S[u4(i, i)]));
        double xs[kXNum];
        xs[kXCost] = S[kPCost];
        xs[kXFail] = S[kPFail];
        xs[kXFixed] = 0.0;       // every residual block touches the free point: no fixed cost
        xs[kXFixedFail] = 0.0;
        xs[kXXnorm2] = point_norm2(x);
        fin_push(s, first, S[kPCost], gmax, xs, 0.0);
      }
      fin_count(s);
    }
    if (!s.done) {
      // LevenbergMarquardtStrategy::ComputeStep on the Jacobi-scaled system: (S H S + D / radius) y = S g
      if (!s.reuse_diag)
#pragma unroll
        for (int i = 0; i < 4; ++i) diag[i] = fmin(fmax(scale[i] * scale[i] * S[u4(i, i)], s.min_diag), s.max_diag);
      double H[4][4], gs[4], L[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = i; j < 4; ++j) H[i][j] = H[j][i] = S[u4(i, j)] * scale[i] * scale[j];
        gs[i] = S[kPG + i] * scale[i];
      }
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double d = H[j][j] + diag[j] / s.radius;
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        if (!(d > 0.0)) ok = false;   // non-positive (or NaN) pivot: the step is invalid
        const double ljj = sqrt(d);
        L[j][j] = ljj;
        const double inv = 1.0 / ljj;
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
          double t = H[i][j];
#pragma unroll
          for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
          L[i][j] = t * inv;
        }
      }
      u[kULinFail] = ok ? 0.0 : 1.0;
      u[kUModel] = u[kUStep2] = u[kUCandX2] = u[kUCandCost] = u[kUCandFail] = 0.0;
      if (ok) {
        double y[4], step[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          double t = gs[i];
#pragma unroll
          for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
          y[i] = t / L[i][i];
        }
#pragma unroll
        for (int i = 3; i >= 0; --i) {
          double t = y[i];
#pragma unroll
          for (int k = i + 1; k < 4; ++k) t -= L[k][i] * y[k];
          y[i] = t / L[i][i];
        }
        // model cost change -(J s) . (r + (J s) / 2) = -(s . g~ + s^T H~ s / 2) from the stored system
        double sg = 0.0, shs = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) step[i] = -y[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          double hs = 0.0;
#pragma unroll
          for (int j = 0; j < 4; ++j) hs += H[i][j] * step[j];
          sg += step[i] * gs[i];
          shs += step[i] * hs;
        }
        u[kUModel] = -(sg + 0.5 * shs);
        double step2 = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          xc[i] = x[i] + step[i] * scale[i];
          step2 += (x[i] - xc[i]) * (x[i] - xc[i]);
        }
        u[kUStep2] = step2;
        u[kUCandX2] = point_norm2(xc);
        eval = true;
      }
    }
    if (!__any(!s.done)) break;   // wave-uniform: the sweep below always runs with all 64 lanes
    double C[kPtNV];              // the linearization at the candidate
    point_linearize(a, R, eval ? cnt : 0, lane, xc, C);
    if (!s.done) {
      if (eval) {
        u[kUCandCost] = C[kPCost];
        u[kUCandFail] = C[kPFail];
      }
      const int cur = s.cur;
      decide_step(s, u, c);
      if (s.cur != cur) {   // accepted: the candidate and its linearization are the current ones
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = xc[i];
#pragma unroll
        for (int j = 0; j < kPtNV; ++j) S[j] = C[j];
      }
    }
  }
  if (run && lane == 0) {
    PointOut o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o.X[i] = x[i];
    o.initial_cost = s.initial_cost;
    o.final_cost = s.min_pushed_cost + s.fixed_cost;
    o.radius = s.radius;
    o.num_iterations = s.pushed;
    o.n_succ = s.n_succ;
    o.n_unsucc = s.n_unsucc;
    o.n_invalid = s.n_invalid;
    o.termination = s.termination;
    o.ok = s.ok;
    o.lm_iters = s.lm_iters;
    o.finished = s.done;
    a.out[pi] = o;
  }
}

// The minimizer's state at the start of a solve, as BaSolver::Begin sets it.
LmState InitialLmState(const sg_solver_options& o) {
  LmState s{};
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
  return s;
}

}  // namespace

void PointSolver::Upload(int32_t n) {
  stream_.Bind();
  io_.Begin();
  io_.Up(off_, plan_.off);
  io_.Up(obs_, plan_.obs);
  io_.Up(frames_, plan_.frames);
  io_.Up(k_, plan_.k);
  io_.Up(points_, plan_.points);
  out_.Resize((size_t)n);
  io_.FlushUp(stream_.get());
}

void PointSolver::LaunchLm(int32_t n, double range, const sg_solver_options& o) {
  PointArgs a{};
  a.off = off_.ptr;
  a.obs = obs_.ptr;
  a.frames = frames_.ptr;
  a.k = k_.ptr;
  a.points = points_.ptr;
  a.out = out_.ptr;
  a.b = range * range;
  a.inv_b = 1.0 / a.b;
  a.n = n;
  // the bound of BaSolver::Solve's host loop: every iteration, rejected and invalid steps included
  const long long cap =
      (long long)std::max(o.max_num_iterations, 0) * (std::max(o.max_num_consecutive_invalid_steps, 0) + 2) + 16;
  a.cap = (int32_t)std::min<long long>(cap, INT_MAX);
  const unsigned grid = (unsigned)((n + kPointsPerBlock - 1) / kPointsPerBlock);
  hipLaunchKernelGGL(k_point_lm, dim3(grid), dim3(kPointThreads), 0, stream_.get(), a, InitialLmState(o));
  SG_HIP_CHECK(hipGetLastError());
}

void PointSolver::Summarize(int32_t i) {
  const PointOut& r = out_h_[i];
  SG_REQUIRE(r.finished, SG_EDEVICE, "LM loop did not terminate on the device");
  sg_solver_summary& su = sums_[i];
  su.num_iterations = r.num_iterations;
  su.num_successful_steps = r.n_succ;
  su.num_unsuccessful_steps = r.n_unsucc;
  su.num_invalid_steps = r.n_invalid;
  su.termination_type = r.termination;
  su.ok = r.ok;
  su.initial_cost = r.initial_cost;
  su.final_cost = r.final_cost;
  su.fixed_cost = 0.0;
  su.trust_region_radius = r.radius;
  su.num_lm_iterations = r.lm_iters;
  su.sync_timeouts = 0;   // nothing to time out on: no hand-off between workgroups
}

void PointSolver::Solve(sg_map* m, const int32_t* points, int32_t n, double range, const sg_solver_options& o,
                        int32_t* solved, sg_solver_summary* summaries) {
  SG_REQUIRE(m && (n == 0 || (points && solved)), SG_EINVAL, "null argument");
  PlanPoints(*m, points, n, &plan_);
  sg_solver_summary none{};
  none.termination_type = SG_DID_NOT_RUN;
  sums_.assign((size_t)n, none);
  for (int i = 0; i < n; ++i) solved[i] = 0;
  timer_.Reset();
  if (plan_.num_run > 0) {
    Upload(n);
    timer_.Start(stream_.get());
    LaunchLm(n, range, o);
    timer_.Stop(stream_.get());
    out_h_.resize((size_t)n);
    io_.Down(out_h_.data(), out_.ptr, (size_t)n * sizeof(PointOut));
    io_.FinishDown(stream_.get());
    timer_.Read();
    for (int i = 0; i < n; ++i)
      if (plan_.points[i].run) Summarize(i);   // (the PointOut of a point that did not run was not written)
    // write-back only after every point's result has been checked: a failed call changes nothing
    for (int i = 0; i < n; ++i) {
      if (!plan_.points[i].run || !sums_[i].ok) continue;
      std::memcpy(m->X + 4 * (size_t)points[i], out_h_[i].X, 4 * sizeof(double));
      solved[i] = 1;
    }
  }
  if (summaries)
    for (int i = 0; i < n; ++i) summaries[i] = sums_[i];
}

}  // namespace sg
