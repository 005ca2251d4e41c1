// ba_pose.hip — pose-only (motion-only) bundle adjustment: sg_slam_solve_frame_poses.
//
// For each requested frame, the Ceres problem Slam::SetupProblem (slam.cpp:257-414) would build if only that
// frame were free: one ReprojectionError + CauchyLoss(range) per usable observation, the frame's quaternion
// (ceres::QuaternionParameterization on Eigen memory, project_math.h) and translation free, every point and the
// intrinsics constant, and optionally FrameDistance(150) + CauchyLoss(15) to the constant translation of the
// previous frame (slam.cpp:86-105, 401-410).  Six unknowns per frame and no coupling between frames, so a whole
// Levenberg-Marquardt solve fits in one workgroup: k_pose_lm runs one workgroup per frame and the entire LM loop
// inside one launch, with no hand-off between workgroups.  The minimizer's bookkeeping (iteration push,
// tolerance tests, step decision, radius update) is ba_lm.h's, the one copy the window solver uses.
//
// Per LM iteration one sweep over the frame's observation records: the candidate x + delta is linearized when it
// is evaluated, so an accepted step's normal equations are already there (a rejected step's are dropped).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>

#include "ba_lm.h"
#include "ba_pose.h"

namespace sg {

namespace {

// A linearization's sums: the 21 upper entries of J^T J (u6 order) | J^T r (6) | cost | behind-camera count
constexpr int kPoseNV = 29;
constexpr int kVG = 21, kVCost = 27, kVFail = 28;

struct PoseArgs {
  const PoseFrame* frames;
  const int32_t* off;
  const double* records;   // PoseRecord as 6 doubles
  PoseOut* out;
  double b, inv_b;                        // CauchyLoss(range): b = range^2
  double fd_target, fd_b2, fd_inv_b2;     // FrameDistance(150), CauchyLoss(15)
  int32_t cap;                            // LM loop bound (a defect ends as an error, not as a hang)
};

// One sweep over the frame's records at pose p (q 4 | t 3): every thread accumulates its records' normal-equation
// terms (records tid, tid + 256, ... in that order), then a fixed-order reduction (DPP wave sums, the four waves
// through LDS in order): sys[kPoseNV] holds the totals, bit for bit the same whatever the grid.
__device__ __forceinline__ void pose_linearize(const double* p, const double* kk, const double (*rec)[kPoseStage],
                                               const double* R, int cnt, double b, double inv_b,
                                               double (*red)[kPoseNV], double* sys) {
  const int tid = threadIdx.x;
  double q[4], t[3], k[7];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = p[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = p[4 + i];
#pragma unroll
  for (int i = 0; i < 7; ++i) k[i] = kk[i];
  double v[kPoseNV];
#pragma unroll
  for (int j = 0; j < kPoseNV; ++j) v[j] = 0.0;
  for (int i = tid; i < cnt; i += kPoseThreads) {
    double pt[2], X[4];
    if (i < kPoseStage) {
      pt[0] = rec[0][i];
      pt[1] = rec[1][i];
#pragma unroll
      for (int a = 0; a < 4; ++a) X[a] = rec[2 + a][i];
    } else {
      const double* r = R + 6 * (size_t)i;
      pt[0] = r[0];
      pt[1] = r[1];
#pragma unroll
      for (int a = 0; a < 4; ++a) X[a] = r[2 + a];
    }
    double r[2], Jc[12], Jp[8], c;
    if (!LinearizeObservation(q, t, k, X, pt, b, inv_b, r, Jc, Jp, &c)) {
      v[kVFail] += 1.0;
      continue;
    }
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int c2 = a; c2 < 6; ++c2) v[e++] += Jc[a] * Jc[c2] + Jc[6 + a] * Jc[6 + c2];
      v[kVG + a] += Jc[a] * r[0] + Jc[6 + a] * r[1];
    }
    v[kVCost] += c;
  }
#pragma unroll
  for (int j = 0; j < kPoseNV; ++j) v[j] = wave_sum_full(v[j]);   // (every thread of the block: all lanes active)
  if ((tid & 63) == 0)
#pragma unroll
    for (int j = 0; j < kPoseNV; ++j) red[tid >> 6][j] = v[j];
  __syncthreads();
  if (tid < kPoseNV) sys[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  __syncthreads();
}

// The FrameDistance block (slam.cpp:86-105) between translation t and the constant tp, added to a linearization's
// sums (thread 0): r = 0.1 (|t - tp| - 150) with CauchyLoss(15), Jacobian on the frame's translation columns.
__device__ __forceinline__ void pose_add_fd(double* sys, const double* t, const double* tp, const PoseArgs& a) {
  const double e[3] = {t[0] - tp[0], t[1] - tp[1], t[2] - tp[2]};
  const double dist = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
  const double r = 0.1 * (dist - a.fd_target);
  double rho0, rho1;
  Cauchy(r * r, a.fd_b2, a.fd_inv_b2, &rho0, &rho1);
  sys[kVCost] += 0.5 * rho0;
  const double sr = sqrt(rho1);
  const double rr = sr * r;
  const double g = 0.1 / dist;
  const double ga[3] = {sr * (g * e[0]), sr * (g * e[1]), sr * (g * e[2])};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = i; j < 3; ++j) sys[u6(3 + i, 3 + j)] += ga[i] * ga[j];
    sys[kVG + 3 + i] += ga[i] * rr;
  }
}

__device__ __forceinline__ double pose_norm2(const double* p) {
  double n = 0.0;
#pragma unroll
  for (int i = 0; i < 7; ++i) n += p[i] * p[i];
  return n;
}

// One workgroup per requested frame; the whole Ceres 1.8 LM loop (TrustRegionMinimizer + LevenbergMarquardtStrategy
// as ba_lm.h restates them) of its 6-unknown problem.
__global__ __launch_bounds__(kPoseThreads) void k_pose_lm(PoseArgs a, LmState init) {
  __shared__ double rec[6][kPoseStage];
  __shared__ double red[kPoseWaves][kPoseNV];
  __shared__ double sys[2][kPoseNV + 3];   // the linearization at pose[slot]
  __shared__ double pose[2][8];            // q 4 | t 3: the current point (LmState::cur) and the candidate
  __shared__ double kk[7], tprev[3];
  __shared__ int ctl[4];                   // done | candidate to evaluate | its slot
  const int tid = threadIdx.x;
  const PoseFrame& fr = a.frames[blockIdx.x];
  if (!fr.run) return;   // (the whole workgroup: fewer than kPoseMinObs records, decided by the planner)
  const int o0 = a.off[blockIdx.x], cnt = a.off[blockIdx.x + 1] - o0;
  const double* R = a.records + 6 * (size_t)o0;
  const int has_dist = fr.has_dist;
  for (int i = tid; i < cnt && i < kPoseStage; i += kPoseThreads) {
    const double* r = R + 6 * (size_t)i;
#pragma unroll
    for (int j = 0; j < 6; ++j) rec[j][i] = r[j];
  }
  if (tid < 4) pose[0][tid] = fr.q[tid];
  if (tid < 3) {
    pose[0][4 + tid] = fr.t[tid];
    tprev[tid] = fr.tprev[tid];
  }
  if (tid < 7) kk[tid] = fr.k[tid];
  __syncthreads();

  pose_linearize(pose[0], kk, rec, R, cnt, a.b, a.inv_b, red, sys[0]);
  if (tid == 0 && has_dist) pose_add_fd(sys[0], pose[0] + 4, tprev, a);

  // thread 0 runs the minimizer on register copies; the other threads only sweep
  LmState s = init;
  double scale[6] = {1, 1, 1, 1, 1, 1}, diag[6] = {0, 0, 0, 0, 0, 0};
  double u[kUNum];
  const double c[kCNum] = {0, 0, 0, 0, 0, 0};   // no second solver stage: the Cholesky's slots stay zero
#pragma unroll
  for (int i = 0; i < kUNum; ++i) u[i] = 0.0;
  for (int it = 0; it < a.cap; ++it) {
    if (tid == 0) {
      const double* S = sys[s.cur];
      const double* x = pose[s.cur];
      if (s.need_lin) {
        double gmax = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) gmax = fmax(gmax, fabs(S[kVG + i]));
        const bool first = s.first;
        if (first && s.jacobi)
#pragma unroll
          for (int i = 0; i < 6; ++i) scale[i] = 1.0 / (1.0 + sqrt(S[u6(i, i)]));
        double xs[kXNum];
        xs[kXCost] = S[kVCost];
        xs[kXFail] = S[kVFail];
        xs[kXFixed] = 0.0;       // every residual block touches the free frame: no fixed cost
        xs[kXFixedFail] = 0.0;
        xs[kXXnorm2] = pose_norm2(x);
        fin_push(s, first, S[kVCost], gmax, xs, 0.0);
      }
      fin_count(s);
      int eval = 0;
      if (!s.done) {
        // LevenbergMarquardtStrategy::ComputeStep on the Jacobi-scaled system: (S H S + D / radius) y = S g
        if (!s.reuse_diag)
#pragma unroll
          for (int i = 0; i < 6; ++i) diag[i] = fmin(fmax(scale[i] * scale[i] * S[u6(i, i)], s.min_diag), s.max_diag);
        double H[6][6], gs[6], L[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int j = i; j < 6; ++j) H[i][j] = H[j][i] = S[u6(i, j)] * scale[i] * scale[j];
          gs[i] = S[kVG + i] * scale[i];
        }
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          double d = H[j][j] + diag[j] / s.radius;
#pragma unroll
          for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
          if (!(d > 0.0)) ok = false;   // non-positive (or NaN) pivot: the step is invalid
          const double ljj = sqrt(d);
          L[j][j] = ljj;
          const double inv = 1.0 / ljj;
#pragma unroll
          for (int i = j + 1; i < 6; ++i) {
            double t = H[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t * inv;
          }
        }
        u[kULinFail] = ok ? 0.0 : 1.0;
        u[kUModel] = u[kUStep2] = u[kUCandX2] = u[kUCandCost] = u[kUCandFail] = 0.0;
        if (ok) {
          double y[6], step[6];
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            double t = gs[i];
#pragma unroll
            for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
            y[i] = t / L[i][i];
          }
#pragma unroll
          for (int i = 5; i >= 0; --i) {
            double t = y[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) t -= L[k][i] * y[k];
            y[i] = t / L[i][i];
          }
          // model cost change -(J s) . (r + (J s) / 2) = -(s . g~ + s^T H~ s / 2) from the stored system
          double sg = 0.0, shs = 0.0;
#pragma unroll
          for (int i = 0; i < 6; ++i) step[i] = -y[i];
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            double hs = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) hs += H[i][j] * step[j];
            sg += step[i] * gs[i];
            shs += step[i] * hs;
          }
          u[kUModel] = -(sg + 0.5 * shs);
          double delta[6];
#pragma unroll
          for (int i = 0; i < 6; ++i) delta[i] = step[i] * scale[i];
          double* xc = pose[s.cur ^ 1];
          double qc[4];
          QuatPlus(x, delta, qc);
          double step2 = 0.0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            xc[i] = qc[i];
            step2 += (x[i] - qc[i]) * (x[i] - qc[i]);
          }
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const double tc = x[4 + i] + delta[3 + i];
            xc[4 + i] = tc;
            step2 += (x[4 + i] - tc) * (x[4 + i] - tc);
          }
          u[kUStep2] = step2;
          u[kUCandX2] = pose_norm2(xc);
          eval = 1;
        }
      }
      ctl[0] = s.done;
      ctl[1] = eval;
      ctl[2] = s.cur ^ 1;
    }
    __syncthreads();
    const int done = ctl[0], eval = ctl[1], cs = ctl[2];
    if (done) break;
    if (eval) pose_linearize(pose[cs], kk, rec, R, cnt, a.b, a.inv_b, red, sys[cs]);
    if (tid == 0) {
      if (eval) {
        if (has_dist) pose_add_fd(sys[cs], pose[cs] + 4, tprev, a);
        u[kUCandCost] = sys[cs][kVCost];
        u[kUCandFail] = sys[cs][kVFail];
      }
      decide_step(s, u, c);   // accepted: s.cur flips to the candidate's slot, whose linearization is sys[cs]
    }
    __syncthreads();   // ctl and the rejected slot are rewritten by the next iteration
  }
  if (tid == 0) {
    PoseOut o;
    const double* x = pose[s.cur];
#pragma unroll
    for (int i = 0; i < 4; ++i) o.q[i] = x[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = x[4 + i];
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
    a.out[blockIdx.x] = o;
  }
}

}  // namespace

void PoseSolver::LaunchLm(int32_t n, double range, const sg_solver_options& o) {
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
  PoseArgs a{};
  a.frames = frames_.ptr;
  a.off = off_.ptr;
  a.records = reinterpret_cast<const double*>(records_.ptr);
  a.out = out_.ptr;
  a.b = range * range;
  a.inv_b = 1.0 / a.b;
  a.fd_target = 150.0;   // FrameDistance(150.) with CauchyLoss(15) (slam.cpp:403-404)
  a.fd_b2 = 15.0 * 15.0;
  a.fd_inv_b2 = 1.0 / a.fd_b2;
  // the bound of BaSolver::Solve's host loop: every iteration, rejected and invalid steps included
  const long long cap =
      (long long)std::max(o.max_num_iterations, 0) * (std::max(o.max_num_consecutive_invalid_steps, 0) + 2) + 16;
  a.cap = (int32_t)std::min<long long>(cap, INT_MAX);
  hipLaunchKernelGGL(k_pose_lm, dim3((unsigned)n), dim3(kPoseThreads), 0, stream_.get(), a, s);
  SG_HIP_CHECK(hipGetLastError());
}

void PoseSolver::Summarize(int i) {
  const PoseOut& r = out_h_[i];
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
  su.fixed_cost = r.fixed_cost;
  su.trust_region_radius = r.radius;
  su.num_lm_iterations = r.lm_iters;
  su.sync_timeouts = 0;   // nothing to time out on: no hand-off between workgroups
}

void PoseSolver::Solve(sg_map* m, const int32_t* frames, int32_t n, double range, bool with_frame_distance,
                       const sg_solver_options& o, int32_t* solved, sg_solver_summary* summaries) {
  SG_REQUIRE(m && (n == 0 || (frames && solved)), SG_EINVAL, "null argument");
  PlanPoses(*m, frames, n, with_frame_distance, &plan_);
  sg_solver_summary none{};
  none.termination_type = SG_DID_NOT_RUN;
  sums_.assign((size_t)n, none);
  for (int i = 0; i < n; ++i) solved[i] = 0;
  timer_.Reset();
  if (plan_.num_run > 0) {
    stream_.Bind();
    io_.Begin();
    io_.Up(frames_, plan_.frames);
    io_.Up(off_, plan_.off);
    io_.Up(records_, plan_.records);
    out_.Resize((size_t)n);
    io_.FlushUp(stream_.get());
    timer_.Start(stream_.get());
    LaunchLm(n, range, o);
    timer_.Stop(stream_.get());
    out_h_.resize((size_t)n);
    io_.Down(out_h_.data(), out_.ptr, (size_t)n * sizeof(PoseOut));
    io_.FinishDown(stream_.get());
    timer_.Read();
    for (int i = 0; i < n; ++i) {
      if (!plan_.frames[i].run) continue;
      Summarize(i);
    }
    // write-back only after every frame's result has been checked: a failed call changes nothing
    for (int i = 0; i < n; ++i) {
      if (!plan_.frames[i].run || !sums_[i].ok) continue;
      std::memcpy(m->q + 4 * (size_t)frames[i], out_h_[i].q, 4 * sizeof(double));
      std::memcpy(m->t + 3 * (size_t)frames[i], out_h_[i].t, 3 * sizeof(double));
      solved[i] = 1;
    }
  }
  if (summaries)
    for (int i = 0; i < n; ++i) summaries[i] = sums_[i];
}

}  // namespace sg
