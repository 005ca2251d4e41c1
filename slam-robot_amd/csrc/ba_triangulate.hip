// ba_triangulate.hip — linear multi-view triangulation: sg_slam_triangulate_points.
//
// Each listed point's location from its enabled observations alone (the location at entry is not read): the
// homogeneous DLT of triangulate_math.h in a local frame, a cheirality test that means what it says because the
// sign is fixed with X.w >= 0 first (the reference's p.z < 0.001 X.w, project.h:27, accepts a point behind every
// camera when W < 0), parallax and reprojection-error gates, and optionally k_point_lm as the polish.
//
// k_point_triangulate has the shape of k_point_lm (ba_points.hip): kPointGroup = 8 consecutive lanes per listed
// point, lane j takes records j, j + 8, ..., no LDS, no barrier, nothing between workgroups.  Three sweeps over
// the point's records: the local frame's unit L^2; the 10 sums of M; the quality sweep at X.  The sums cross the
// group by sum8_dpp and the two maxima by max8_dpp, which leave identical bits in all 8 lanes, so the Jacobi
// eigen-solve, the sign rule and the status run redundantly in every lane and nothing is broadcast; lane 0 writes.
// Every sweep runs under a full EXEC mask: idle, padding and DID_NOT_RUN groups, and groups that already have
// their status, enter it with a count of 0.
#include <hip/hip_runtime.h>

#include <cstring>

#include "ba_device.h"
#include "ba_points.h"
#include "triangulate_math.h"

namespace sg {

namespace {

struct TriArgs {
  const int32_t* off;
  const PointObs* obs;
  const PointFrame* frames;
  const double* k;
  PointStart* points;            // written when refine: X and run of the start k_point_lm reads
  sg_triangulate_result* out;
  double min_parallax, max_error_px;
  int32_t n;
  int32_t refine;
};

struct TriRecord {
  double q[4], t[3], k[7], pt[2];
};

__device__ __forceinline__ TriRecord tri_load(const TriArgs& a, const PointObs* R, int i) {
  const PointObs ob = R[i];
  const PointFrame& fr = a.frames[ob.frame];
  const double* kp = a.k + 7 * (size_t)fr.camera;
  TriRecord r;
#pragma unroll
  for (int c = 0; c < 4; ++c) r.q[c] = fr.q[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) r.t[c] = fr.t[c];
#pragma unroll
  for (int c = 0; c < 7; ++c) r.k[c] = kp[c];
  r.pt[0] = ob.u;
  r.pt[1] = ob.v;
  return r;
}

__global__ __launch_bounds__(kPointThreads) void k_point_triangulate(TriArgs a) {
  const int gid = blockIdx.x * kPointThreads + threadIdx.x;
  const int pi = gid / kPointGroup, lane = gid % kPointGroup;
  const bool listed = pi < a.n;
  const bool run = listed && a.points[listed ? pi : 0].run != 0;
  const int o0 = run ? a.off[pi] : 0, cnt = run ? a.off[pi + 1] - o0 : 0;
  const PointObs* R = a.obs + o0;
  // the first record's pose: the local frame's origin, the sign rule's camera, the parallax's other ray
  double q0[4] = {0, 0, 0, 1}, t0[3] = {0, 0, 0};
  if (run) {
    const PointFrame& f0 = a.frames[R[0].frame];
#pragma unroll
    for (int c = 0; c < 4; ++c) q0[c] = f0.q[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) t0[c] = f0.t[c];
  }
  int status = run ? SG_TRI_OK : SG_TRI_DID_NOT_RUN;
  bool go = run;

  // sweep 1: L^2 = mean |t_i - c0|^2
  double l2 = 0.0;
  for (int i = lane; i < cnt; i += kPointGroup) l2 += TriCentreDist2(a.frames[R[i].frame].t, t0);
  l2 = sum8_dpp(l2);
  if (go) {
    l2 /= (double)cnt;
    if (l2 == 0.0) {
      status = SG_TRI_NO_BASELINE;
      go = false;
    }
  }
  const double l = go ? sqrt(l2) : 1.0, inv_l = 1.0 / l;

  // sweep 2: M
  double M[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) M[j] = 0.0;
  for (int i = lane, n2 = go ? cnt : 0; i < n2; i += kPointGroup) {
    const TriRecord r = tri_load(a, R, i);
    TriAddRows(r.q, r.t, r.k, r.pt, t0, inv_l, M);
  }
#pragma unroll
  for (int j = 0; j < 10; ++j) M[j] = sum8_dpp(M[j]);

  double X[4] = {0, 0, 0, 0}, rel_gap = 0.0;
  if (go) {
    double lam[4], y[4];
    TriJacobi4(M, lam, y);
    status = TriEigenStatus(lam, y);
    if (status == SG_TRI_OK) {
      rel_gap = TriRelGap(lam);
      TriToWorld(y, t0, l, q0, t0, X);
    } else {
      go = false;
    }
  }

  // sweep 3: quality at X
  double behind = 0.0, err = 0.0, par = 0.0;
  for (int i = lane, n3 = go ? cnt : 0; i < n3; i += kPointGroup) {
    const TriRecord r = tri_load(a, R, i);
    TriQuality(r.q, r.t, r.k, r.pt, t0, X, &behind, &err, &par);
  }
  behind = sum8_dpp(behind);
  err = max8_dpp(err);
  par = max8_dpp(par);
  if (go) {
    status = TriGateStatus(X, behind, err, par, a.min_parallax, a.max_error_px);
    if (status == SG_TRI_DEGENERATE) go = false;
  }

  if (run && lane == 0) {
    sg_triangulate_result o;
    o.status = status;
    o.num_obs = cnt;
    o.parallax = go ? par : 0.0;
    o.max_error_px = go ? err : 0.0;
    o.rel_gap = rel_gap;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.X[j] = go ? X[j] : 0.0;
    a.out[pi] = o;
    if (a.refine) {
      PointStart ps;
#pragma unroll
      for (int j = 0; j < 4; ++j) ps.X[j] = X[j];
      ps.run = status == SG_TRI_OK;
      ps.pad = 0;
      a.points[pi] = ps;
    }
  }
}

}  // namespace

void PointSolver::Triangulate(sg_map* m, const int32_t* points, int32_t n, const sg_triangulate_options& t,
                              const sg_solver_options& o, int32_t* solved, sg_triangulate_result* results,
                              sg_solver_summary* summaries) {
  SG_REQUIRE(m && (n == 0 || (points && solved)), SG_EINVAL, "null argument");
  PlanPoints(*m, points, n, &plan_);
  sg_solver_summary none{};
  none.termination_type = SG_DID_NOT_RUN;
  sums_.assign((size_t)n, none);
  tri_.assign((size_t)n, sg_triangulate_result{});
  for (int i = 0; i < n; ++i) {
    tri_[i].status = SG_TRI_DID_NOT_RUN;
    tri_[i].num_obs = plan_.off[i + 1] - plan_.off[i];
  }
  timer_.Reset();
  const bool refine = t.refine != 0;
  if (plan_.num_run > 0) {
    Upload(n);
    tri_d_.Resize((size_t)n);
    TriArgs a{};
    a.off = off_.ptr;
    a.obs = obs_.ptr;
    a.frames = frames_.ptr;
    a.k = k_.ptr;
    a.points = points_.ptr;
    a.out = tri_d_.ptr;
    a.min_parallax = t.min_parallax;
    a.max_error_px = t.max_error_px;
    a.n = n;
    a.refine = refine;
    timer_.Start(stream_.get());
    const unsigned grid = (unsigned)((n + kPointsPerBlock - 1) / kPointsPerBlock);
    hipLaunchKernelGGL(k_point_triangulate, dim3(grid), dim3(kPointThreads), 0, stream_.get(), a);
    SG_HIP_CHECK(hipGetLastError());
    // the polish reads the PointStart array the launch above rewrote: run = 1 for exactly the SG_TRI_OK points
    if (refine) LaunchLm(n, t.range, o);
    timer_.Stop(stream_.get());
    tri_h_.resize((size_t)n);
    io_.Down(tri_h_.data(), tri_d_.ptr, (size_t)n * sizeof(sg_triangulate_result));
    if (refine) {
      out_h_.resize((size_t)n);
      io_.Down(out_h_.data(), out_.ptr, (size_t)n * sizeof(PointOut));
    }
    io_.FinishDown(stream_.get());
    timer_.Read();
    for (int i = 0; i < n; ++i) {
      if (!plan_.points[i].run) continue;   // (its result was not written)
      const sg_triangulate_result& r = tri_h_[i];
      SG_REQUIRE(r.status == SG_TRI_OK || (r.status >= SG_TRI_NO_BASELINE && r.status <= SG_TRI_HIGH_ERROR),
                 SG_EDEVICE, "triangulation status out of range");
      SG_REQUIRE(r.num_obs == tri_[i].num_obs, SG_EDEVICE, "triangulation result of another point");
      tri_[i] = r;
      if (refine && r.status == SG_TRI_OK) Summarize(i);
    }
  }
  // write-back only after every point's result has been checked: a failed call changes nothing
  for (int i = 0; i < n; ++i) {
    solved[i] = tri_[i].status == SG_TRI_OK;
    if (!solved[i]) continue;
    const double* X = refine && sums_[i].ok ? out_h_[i].X : tri_[i].X;
    std::memcpy(m->X + 4 * (size_t)points[i], X, 4 * sizeof(double));
  }
  if (results)
    for (int i = 0; i < n; ++i) results[i] = tri_[i];
  if (summaries)
    for (int i = 0; i < n; ++i) summaries[i] = sums_[i];
}

}  // namespace sg
