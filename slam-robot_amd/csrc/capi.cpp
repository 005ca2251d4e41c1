// capi.cpp — extern "C" entry points of libslamgpu.so (include/slamgpu.h).
//
// sg_ba_*   : the device solver (Ceres 1.8 LM + SPARSE_SCHUR restated on MI355X, slam.cpp:482-521)
// sg_slam_* : the Slam object of slam.h:21-65 — SolveFrames / SolveAllFrames / ReprojectMap with
//             iterations() and error() bookkeeping — on top of sg_problem_* and sg_ba_*.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "ba_align.h"
#include "ba_epipolar.h"
#include "ba_match.h"
#include "ba_points.h"
#include "ba_pose.h"
#include "ba_posegraph.h"
#include "ba_relpose.h"
#include "ba_solver.h"
#include "comm.h"
#include "common.h"
#include "map_ops.h"

struct sg_ba {
  std::unique_ptr<sg::BaSolver> solver;
};

struct sg_comm_group {
  std::shared_ptr<sg::LocalGroup> g;
};

struct sg_slam {
  std::unique_ptr<sg::BaSolver> solver;
  std::unique_ptr<sg::MapOps> mapops;   // created on first use
  std::unique_ptr<sg::PoseSolver> pose;  // created on first use (sg_slam_solve_frame_poses)
  std::unique_ptr<sg::PointSolver> points;   // created on first use (sg_slam_solve_points)
  std::unique_ptr<sg::RelPoseSolver> relpose;   // created on first use (sg_slam_relative_poses)
  std::unique_ptr<sg::AlignSolver> align;   // created on first use (sg_slam_align_points)
  std::unique_ptr<sg::PoseGraphSolver> posegraph;   // created on first use (sg_slam_optimize_pose_graph)
  std::unique_ptr<sg::MatchSolver> match;   // created on first use (sg_slam_match_by_projection)
  std::unique_ptr<sg::EpipolarSolver> epipolar;   // created on first use (sg_slam_match_epipolar)
  sg_device_options dev;
  sg_solver_options options;
  int32_t iterations = 0;    // Slam::iterations_ (slam.cpp:517)
  double error = 0.0;        // Slam::error_ (slam.cpp:518)
  sg_solver_summary last{};
  double phase_ms[4] = {0, 0, 0, 0};   // last SolveFrames / SolveAllFrames: setup, load, solve, write-back
  int32_t res_f = 0, res_p = 0, res_m = 0;   // buffers reserved for a map of this size (high-water mark)
};

extern "C" {

int sg_ba_create(sg_ba** out, const sg_device_options* dev) {
  SG_CAPI_BEGIN
  SG_REQUIRE(out, SG_EINVAL, "null output handle");
  sg_device_options d;
  sg_device_options_default(&d);
  if (dev) d = *dev;
  auto h = std::make_unique<sg_ba>();
  h->solver.reset(new sg::BaSolver(d));
  *out = h.release();
  SG_CAPI_END
}

void sg_ba_destroy(sg_ba* h) { delete h; }

int sg_comm_unique_id(void* id128) {
  SG_CAPI_BEGIN
  SG_REQUIRE(id128, SG_EINVAL, "null id buffer");
  sg::BaSolver::UniqueId(id128);
  SG_CAPI_END
}

int sg_ba_comm_init(sg_ba* h, const void* id128, int32_t nranks, int32_t rank) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && id128, SG_EINVAL, "null argument");
  h->solver->CommInit(id128, nranks, rank);
  SG_CAPI_END
}

int sg_comm_group_create(sg_comm_group** out, int32_t nranks) {
  SG_CAPI_BEGIN
  SG_REQUIRE(out && nranks >= 1 && nranks <= sg::LocalGroup::kMaxRanks, SG_EINVAL, "bad group size");
  auto g = std::make_unique<sg_comm_group>();
  g->g = std::make_shared<sg::LocalGroup>(nranks);
  *out = g.release();
  SG_CAPI_END
}

void sg_comm_group_destroy(sg_comm_group* g) { delete g; }

int sg_ba_comm_init_local(sg_ba* h, sg_comm_group* g, int32_t rank) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && g, SG_EINVAL, "null argument");
  h->solver->CommInitLocal(g->g, rank);
  SG_CAPI_END
}

int sg_ba_comm_init_host(sg_ba* h, int32_t nranks, int32_t rank, sg_allreduce_fn fn, void* user) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && fn, SG_EINVAL, "null argument");
  h->solver->CommInitHost(nranks, rank, fn, user);
  SG_CAPI_END
}

int sg_ba_load(sg_ba* h, const sg_problem* p) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && p, SG_EINVAL, "null argument");
  h->solver->Load(*p);
  SG_CAPI_END
}

int sg_ba_reserve(sg_ba* h, int32_t max_frames, int32_t max_points, int32_t max_obs) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h, SG_EINVAL, "null handle");
  h->solver->Reserve(max_frames, max_points, max_obs);
  SG_CAPI_END
}

int sg_ba_info_get(const sg_ba* h, sg_ba_info* out) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && out, SG_EINVAL, "null argument");
  h->solver->Info(out);
  SG_CAPI_END
}

int sg_ba_load_counts(const sg_ba* h, int32_t* full_loads, int32_t* value_loads) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && full_loads && value_loads, SG_EINVAL, "null argument");
  h->solver->LoadCounts(full_loads, value_loads);
  SG_CAPI_END
}

int sg_ba_solve(sg_ba* h, const sg_solver_options* o, sg_problem* p, sg_solver_summary* s) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && p && s, SG_EINVAL, "null argument");
  sg_solver_options opt;
  sg_solver_options_default(&opt);
  if (o) opt = *o;
  h->solver->Solve(opt, p, s);
  SG_CAPI_END
}

int sg_ba_begin(sg_ba* h, const sg_solver_options* o) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h, SG_EINVAL, "null handle");
  sg_solver_options opt;
  sg_solver_options_default(&opt);
  if (o) opt = *o;
  h->solver->Begin(opt);
  SG_CAPI_END
}

int sg_ba_iterate(sg_ba* h, int32_t n) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && n >= 0, SG_EINVAL, "bad argument");
  h->solver->Iterate(n);
  SG_CAPI_END
}

int sg_ba_sync(sg_ba* h) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h, SG_EINVAL, "null handle");
  h->solver->Sync();
  SG_CAPI_END
}

int sg_ba_summary(sg_ba* h, sg_solver_summary* s) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && s, SG_EINVAL, "null argument");
  h->solver->Summary(s);
  SG_CAPI_END
}

int sg_ba_download(sg_ba* h, sg_problem* p) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && p, SG_EINVAL, "null argument");
  h->solver->Download(p);
  SG_CAPI_END
}

int sg_ba_set_timing(sg_ba* h, int32_t enable) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h, SG_EINVAL, "null handle");
  h->solver->SetTiming(enable != 0);
  SG_CAPI_END
}

int sg_ba_kernel_times(sg_ba* h, char* names, int32_t names_len, double* ms, int32_t* counts, int32_t max) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && ms && counts, SG_EINVAL, "null argument");
  h->solver->KernelTimes(names, names_len, ms, counts, max);
  SG_CAPI_END
}

int sg_ba_kernel_work(sg_ba* h, double* bytes, double* flops, int32_t max) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && bytes && flops, SG_EINVAL, "null argument");
  h->solver->KernelWork(bytes, flops, max);
  SG_CAPI_END
}

int sg_ba_sweep(sg_ba* h, int32_t n) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && n >= 0, SG_EINVAL, "bad argument");
  h->solver->Sweep(n);
  SG_CAPI_END
}

// Diagnostic (not in the public header): per-phase cycle counters of stamped kernels when SG_STAMP=1.
int sg_ba_debug_stamps(sg_ba* h, unsigned long long* out, int32_t n) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && out, SG_EINVAL, "null argument");
  auto v = h->solver->Stamps();
  for (int32_t i = 0; i < n && i < (int32_t)v.size(); ++i) out[i] = v[i];
  SG_CAPI_END
}

int sg_ba_evaluate(sg_ba* h, double* residuals, double* cost, int32_t* num_failed) {
  SG_CAPI_BEGIN
  SG_REQUIRE(h && residuals && cost && num_failed, SG_EINVAL, "null argument");
  h->solver->Evaluate(residuals, cost, num_failed);
  SG_CAPI_END
}

// ------------------------------------------------------------------------------------------------
// Slam facade

int sg_slam_create(sg_slam** out, const sg_device_options* dev) {
  SG_CAPI_BEGIN
  SG_REQUIRE(out, SG_EINVAL, "null output handle");
  sg_device_options d;
  sg_device_options_default(&d);
  if (dev) d = *dev;
  auto s = std::make_unique<sg_slam>();
  s->solver.reset(new sg::BaSolver(d));
  s->dev = d;
  sg_solver_options_default(&s->options);
  *out = s.release();
  SG_CAPI_END
}

void sg_slam_destroy(sg_slam* s) { delete s; }

int sg_slam_set_options(sg_slam* s, const sg_solver_options* o) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && o, SG_EINVAL, "null argument");
  s->options = *o;
  SG_CAPI_END
}

static void RunProblem(sg_slam* s, sg_problem* p, sg_map* map, const sg_solver_options& o, int32_t* solved) {
  static const bool timing = getenv("SG_HOST_TIMING") != nullptr;   // development aid: phase times to stderr
  auto now = [] { return std::chrono::steady_clock::now(); };
  const auto t0 = now();
  // Reserve device and pinned buffers for twice the largest window problem seen so far, so that they do not
  // grow inside the loads of the calls that follow.  main.cpp's windows (SolveFrames(2, 5), (10, 20)) stay
  // about the same size while the map grows by a frame per call, so after the first calls of each kind no
  // load reallocates.  (Reserving for the whole map, with a quarter's headroom, re-reserved every time the
  // map grew by a quarter: a 5-20 ms hipFree / hipMalloc / hipHostMalloc round in one call out of ten of the
  // replay, tools/e2e_replay.py.)
  (void)map;
  if (p->num_frames > s->res_f || p->num_points > s->res_p || p->num_obs > s->res_m) {
    s->res_f = std::max(s->res_f, 2 * p->num_frames + 4);
    s->res_p = std::max(s->res_p, 2 * p->num_points + 64);
    s->res_m = std::max(s->res_m, 2 * p->num_obs + 512);
    s->solver->Reserve(s->res_f, s->res_p, s->res_m);
    if (timing) fprintf(stderr, "[sg] reserve frames %d points %d observations %d\n", s->res_f, s->res_p, s->res_m);
  }
  s->solver->Load(*p);
  const auto t1 = now();
  sg_solver_summary sum{};
  s->solver->Solve(o, p, &sum);
  const auto t2 = now();
  if (sg_problem_write_back(p, map) != SG_OK) throw sg::Error(SG_EINVAL, sg_last_error());
  const auto t3 = now();
  const auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  s->phase_ms[1] = ms(t0, t1);
  s->phase_ms[2] = ms(t1, t2);
  s->phase_ms[3] = ms(t2, t3);
  if (timing)
    fprintf(stderr, "[sg] load %.2f ms, solve %.2f ms, write-back %.2f ms\n", ms(t0, t1), ms(t1, t2), ms(t2, t3));
  s->iterations += sum.num_iterations;   // iterations_ += summary.iterations.size()
  s->error = sum.final_cost;             // error_ = summary.final_cost
  s->last = sum;
  *solved = sum.ok;                      // summary.error.size() == 0
}

int sg_slam_solve_frames(sg_slam* s, sg_map* map, int32_t num_to_solve, int32_t num_to_present, double range,
                         int32_t* solved) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && solved, SG_EINVAL, "null argument");
  *solved = 0;
  sg_problem p{};
  int32_t built = 0;
  const auto ts = std::chrono::steady_clock::now();
  int rc = sg_problem_from_map_frames(map, num_to_solve, num_to_present, range, &p, &built);
  if (rc != SG_OK) return rc;
  s->phase_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts).count();
  for (int i = 1; i < 4; ++i) s->phase_ms[i] = 0.0;
  if (!built) return SG_OK;   // "Slam aborted due to frame set too small": SolveFrames returns false
  try {
    RunProblem(s, &p, map, s->options, solved);   // Run(false)
  } catch (...) {
    sg_problem_free(&p);
    throw;
  }
  sg_problem_free(&p);
  SG_CAPI_END
}

int sg_slam_solve_all_frames(sg_slam* s, sg_map* map, double range, int32_t solve_cameras, int32_t* solved) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && solved, SG_EINVAL, "null argument");
  *solved = 0;
  sg_problem p{};
  int32_t built = 0;
  const auto ts = std::chrono::steady_clock::now();
  int rc = sg_problem_from_map_all(map, range, solve_cameras, &p, &built);
  if (rc != SG_OK) return rc;
  s->phase_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts).count();
  for (int i = 1; i < 4; ++i) s->phase_ms[i] = 0.0;
  if (!built) return SG_OK;
  sg_solver_options o = s->options;
  if (solve_cameras) o.function_tolerance = 1e-9;   // Run(fine = solve_cameras), slam.cpp:496-499
  try {
    RunProblem(s, &p, map, o, solved);
  } catch (...) {
    sg_problem_free(&p);
    throw;
  }
  sg_problem_free(&p);
  SG_CAPI_END
}

int sg_slam_last_phase_ms(const sg_slam* s, double* ms4) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && ms4, SG_EINVAL, "null argument");
  for (int i = 0; i < 4; ++i) ms4[i] = s->phase_ms[i];
  SG_CAPI_END
}

int sg_slam_reproject_map(sg_slam* s, sg_map* map, double* mean) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && mean, SG_EINVAL, "null argument");
  *mean = s->solver->ReprojectMap(map);
  SG_CAPI_END
}

static sg::MapOps& MapOpsOf(sg_slam* s) {
  if (!s->mapops) s->mapops.reset(new sg::MapOps(s->dev, s->solver->stream()));   // one stream per Slam object
  return *s->mapops;
}

int sg_map_clean(sg_slam* s, sg_map* map, double error_threshold, int32_t* result) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && result, SG_EINVAL, "null argument");
  *result = MapOpsOf(s).Clean(map, error_threshold);
  SG_CAPI_END
}

int sg_map_apply_epipolar(sg_slam* s, sg_map* map, int32_t* num_violations) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && num_violations, SG_EINVAL, "null argument");
  *num_violations = MapOpsOf(s).ApplyEpipolarConstraint(map);
  SG_CAPI_END
}

int sg_map_normalize(sg_slam* s, sg_map* map) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map, SG_EINVAL, "null argument");
  MapOpsOf(s).Normalize(map);
  SG_CAPI_END
}

static sg::PoseSolver& PoseSolverOf(sg_slam* s) {
  if (!s->pose) s->pose.reset(new sg::PoseSolver(s->dev, s->solver->stream()));   // one stream per Slam object
  return *s->pose;
}

int sg_slam_solve_frame_poses(sg_slam* s, sg_map* map, const int32_t* frames, int32_t n, double range,
                              int32_t with_frame_distance, int32_t* solved, sg_solver_summary* summaries) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map, SG_EINVAL, "null argument");
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative frame count");
  if (n == 0) return SG_OK;   // nothing to solve: neither the handle nor the device is touched
  SG_REQUIRE(frames && solved, SG_EINVAL, "null frame list or result array");
  sg::PoseSolver& ps = PoseSolverOf(s);
  ps.Solve(map, frames, n, range, with_frame_distance != 0, s->options, solved, summaries);
  // Slam::Run's bookkeeping (slam.cpp:517-518) over the frames that ran, in list order
  for (const sg_solver_summary& sum : ps.summaries()) {
    if (sum.termination_type == SG_DID_NOT_RUN) continue;
    s->iterations += sum.num_iterations;
    s->error = sum.final_cost;
    s->last = sum;
  }
  SG_CAPI_END
}

int sg_slam_localize_frames(sg_slam* s, sg_map* map, const int32_t* frames, int32_t n,
                            const sg_localize_options* options, int32_t* solved, sg_localize_result* results,
                            int32_t* obs_inlier, sg_solver_summary* summaries) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && options, SG_EINVAL, "null argument");
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative frame count");
  SG_REQUIRE(options->threshold_px > 0.0, SG_EINVAL, "threshold_px must be positive");
  SG_REQUIRE(options->max_hypotheses > 0, SG_EINVAL, "max_hypotheses must be positive");
  if (n == 0) return SG_OK;   // nothing to localize: neither the handle nor the device is touched
  SG_REQUIRE(frames && solved, SG_EINVAL, "null frame list or result array");
  sg::PoseSolver& ps = PoseSolverOf(s);
  ps.Localize(map, frames, n, *options, s->options, solved, results, obs_inlier, summaries);
  // Slam::Run's bookkeeping (slam.cpp:517-518) over the frames the polish ran on, in list order
  for (const sg_solver_summary& sum : ps.summaries()) {
    if (sum.termination_type == SG_DID_NOT_RUN) continue;
    s->iterations += sum.num_iterations;
    s->error = sum.final_cost;
    s->last = sum;
  }
  SG_CAPI_END
}

// Diagnostics (not in the public header): HIP-event time of the k_pose_lm launch (tools/pose_bench.py); after
// sg_slam_localize_frames, of its two to four launches (tools/localize_bench.py).
int sg_slam_debug_pose_timing(sg_slam* s, int32_t enable) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s, SG_EINVAL, "null handle");
  PoseSolverOf(s).SetTiming(enable != 0);
  SG_CAPI_END
}

int sg_slam_debug_pose_kernel_ms(sg_slam* s, double* ms) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && ms, SG_EINVAL, "null argument");
  *ms = PoseSolverOf(s).last_kernel_ms();
  SG_CAPI_END
}

static sg::RelPoseSolver& RelPoseSolverOf(sg_slam* s) {
  if (!s->relpose) s->relpose.reset(new sg::RelPoseSolver(s->dev, s->solver->stream()));   // one stream per Slam object
  return *s->relpose;
}

int sg_slam_relative_poses(sg_slam* s, sg_map* map, const int32_t* pairs, int32_t n, const sg_relpose_options* options,
                           int32_t* solved, sg_relpose_result* results, int32_t* rec_offset, int32_t* rec_inlier,
                           int32_t* rec_obs, int32_t rec_capacity) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && options, SG_EINVAL, "null argument");
  sg::RelPlan plan;
  sg::PlanRelPoses(map, pairs, n, options, &plan);   // every argument check, on the host
  if (n == 0) return SG_OK;   // nothing to solve: neither the handle nor the device is touched
  SG_REQUIRE(solved, SG_EINVAL, "null result array");
  SG_REQUIRE(!(rec_inlier || rec_obs) || rec_capacity >= plan.off[n], SG_EINVAL,
             "rec_capacity is below the call's records");
  RelPoseSolverOf(s).Solve(map, plan, n, *options, solved, results, rec_offset, rec_inlier, rec_obs);
  SG_CAPI_END
}

// Diagnostics (not in the public header): HIP-event time of sg_slam_relative_poses' two launches
// (tools/relpose_bench.py).
int sg_slam_debug_relpose_timing(sg_slam* s, int32_t enable) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s, SG_EINVAL, "null handle");
  RelPoseSolverOf(s).SetTiming(enable != 0);
  SG_CAPI_END
}

int sg_slam_debug_relpose_kernel_ms(sg_slam* s, double* ms) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && ms, SG_EINVAL, "null argument");
  *ms = RelPoseSolverOf(s).last_kernel_ms();
  SG_CAPI_END
}

static sg::AlignSolver& AlignSolverOf(sg_slam* s) {
  if (!s->align) s->align.reset(new sg::AlignSolver(s->dev, s->solver->stream()));   // one stream per Slam object
  return *s->align;
}

int sg_slam_align_points(sg_slam* s, sg_map* map, const int32_t* corr, const int32_t* group_offset, int32_t n,
                         const sg_align_options* options, int32_t* solved, sg_align_result* results,
                         int32_t* corr_inlier) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && options, SG_EINVAL, "null argument");
  sg::AlignPlan plan;
  sg::PlanAlign(map, corr, group_offset, n, options, &plan);   // every argument check, on the host
  if (n == 0) return SG_OK;   // nothing to align: neither the handle nor the device is touched
  SG_REQUIRE(solved, SG_EINVAL, "null result array");
  AlignSolverOf(s).Solve(plan, n, group_offset[n], *options, solved, results, corr_inlier);
  SG_CAPI_END
}

// Diagnostics (not in the public header): HIP-event time of sg_slam_align_points' two launches
// (tools/align_bench.py).
int sg_slam_debug_align_timing(sg_slam* s, int32_t enable) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s, SG_EINVAL, "null handle");
  AlignSolverOf(s).SetTiming(enable != 0);
  SG_CAPI_END
}

int sg_slam_debug_align_kernel_ms(sg_slam* s, double* ms) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && ms, SG_EINVAL, "null argument");
  *ms = AlignSolverOf(s).last_kernel_ms();
  SG_CAPI_END
}

static sg::MatchSolver& MatchSolverOf(sg_slam* s) {
  if (!s->match) s->match.reset(new sg::MatchSolver(s->dev, s->solver->stream()));   // one stream per Slam object
  return *s->match;
}

int sg_slam_match_by_projection(sg_slam* s, const sg_map* map, const int32_t* frames, int32_t n,
                                const int32_t* kp_offset, const double* kp_xy, const uint64_t* kp_desc,
                                const int32_t* points, int32_t np, const uint64_t* point_desc,
                                const sg_match_options* options, int32_t* match, int32_t* best_point,
                                int32_t* best_dist, int32_t* second_dist, int32_t* num_candidates,
                                sg_match_result* results) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && options && match, SG_EINVAL, "null argument");
  sg::MatchPlan plan;
  sg::PlanMatch(map, frames, n, kp_offset, kp_xy, kp_desc, points, np, point_desc, options,
                &plan);   // every argument check, on the host
  if (n == 0) return SG_OK;   // nothing to match: neither the handle nor the device is touched
  const size_t K = (size_t)plan.K;
  // the empty answers; with K == 0 or np == 0 they stand, and the device is not touched
  std::vector<int32_t> bp(K, -1), bd(K, -1), sd(K, -1), nc(K, 0), proj((size_t)n, 0), mt(K, -1);
  if (plan.launch)
    MatchSolverOf(s).Run(plan, kp_xy, kp_desc, points, point_desc, *options, bp.data(), bd.data(), sd.data(), nc.data(),
                         proj.data());
  std::vector<sg_match_result> res((size_t)n, sg_match_result{});
  for (int i = 0; i < n; ++i) {
    res[i].num_keypoints = kp_offset[i + 1] - kp_offset[i];
    res[i].num_projected = proj[i];
  }
  sg::ResolveMatches(kp_offset, n, bp.data(), bd.data(), sd.data(), nc.data(), *options, mt.data(), res.data());
  std::copy(mt.begin(), mt.end(), match);
  if (best_point) std::copy(bp.begin(), bp.end(), best_point);
  if (best_dist) std::copy(bd.begin(), bd.end(), best_dist);
  if (second_dist) std::copy(sd.begin(), sd.end(), second_dist);
  if (num_candidates) std::copy(nc.begin(), nc.end(), num_candidates);
  if (results) std::copy(res.begin(), res.end(), results);
  SG_CAPI_END
}

// Diagnostics (not in the public header): HIP-event time of sg_slam_match_by_projection's three launches
// (tools/match_bench.py).
int sg_slam_debug_match_timing(sg_slam* s, int32_t enable) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s, SG_EINVAL, "null handle");
  MatchSolverOf(s).SetTiming(enable != 0);
  SG_CAPI_END
}

int sg_slam_debug_match_kernel_ms(sg_slam* s, double* ms) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && ms, SG_EINVAL, "null argument");
  *ms = MatchSolverOf(s).last_kernel_ms();
  SG_CAPI_END
}

static sg::EpipolarSolver& EpipolarSolverOf(sg_slam* s) {
  if (!s->epipolar) s->epipolar.reset(new sg::EpipolarSolver(s->dev, s->solver->stream()));   // one stream per Slam object
  return *s->epipolar;
}

// sg_slam_match_epipolar with the device (s) or with the planner's CPU executor (s == nullptr).
static void MatchEpipolar(sg_slam* s, const sg_map* map, const int32_t* pairs, int32_t n, const int32_t* a_offset,
                          const double* a_xy, const uint64_t* a_desc, const int32_t* a_level, const int32_t* b_offset,
                          const double* b_xy, const uint64_t* b_desc, const int32_t* b_level,
                          const sg_epipolar_options* options, int32_t* match, int32_t* best_kp, int32_t* best_dist,
                          int32_t* second_dist, int32_t* num_candidates, sg_epipolar_result* results) {
  sg::EpipolarPlan plan;
  sg::PlanEpipolar(map, pairs, n, a_offset, a_xy, a_desc, a_level, b_offset, b_xy, b_desc, b_level, options,
                   &plan);   // every argument check, on the host
  if (n == 0) return;   // nothing to match: neither the handle nor the device is touched
  const size_t KA = (size_t)plan.KA;
  // the empty answers; when no pair is live they stand, and the device is not touched
  std::vector<int32_t> bk(KA, -1), bd(KA, -1), sd(KA, -1), nc(KA, 0), mt(KA, -1);
  if (!s)
    sg::RunEpipolarCpu(plan, a_offset, a_xy, a_desc, a_level, b_offset, b_xy, b_desc, b_level, *options, bk.data(),
                       bd.data(), sd.data(), nc.data());
  else if (plan.launch)
    EpipolarSolverOf(s).Run(plan, a_offset, a_xy, a_desc, a_level, b_offset, b_xy, b_desc, b_level, *options, bk.data(),
                            bd.data(), sd.data(), nc.data());
  std::vector<sg_epipolar_result> res((size_t)n, sg_epipolar_result{});
  sg::ResolveEpipolar(plan, a_offset, b_offset, bk.data(), bd.data(), sd.data(), nc.data(), *options, mt.data(),
                      res.data());
  std::copy(mt.begin(), mt.end(), match);
  if (best_kp) std::copy(bk.begin(), bk.end(), best_kp);
  if (best_dist) std::copy(bd.begin(), bd.end(), best_dist);
  if (second_dist) std::copy(sd.begin(), sd.end(), second_dist);
  if (num_candidates) std::copy(nc.begin(), nc.end(), num_candidates);
  if (results) std::copy(res.begin(), res.end(), results);
}

int sg_slam_match_epipolar(sg_slam* s, const sg_map* map, const int32_t* pairs, int32_t n, const int32_t* a_offset,
                           const double* a_xy, const uint64_t* a_desc, const int32_t* a_level, const int32_t* b_offset,
                           const double* b_xy, const uint64_t* b_desc, const int32_t* b_level,
                           const sg_epipolar_options* options, int32_t* match, int32_t* best_kp, int32_t* best_dist,
                           int32_t* second_dist, int32_t* num_candidates, sg_epipolar_result* results) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && options && match, SG_EINVAL, "null argument");
  MatchEpipolar(s, map, pairs, n, a_offset, a_xy, a_desc, a_level, b_offset, b_xy, b_desc, b_level, options, match,
                best_kp, best_dist, second_dist, num_candidates, results);
  SG_CAPI_END
}

// Diagnostics (not in the public header): HIP-event time of sg_slam_match_epipolar's three launches, and the same call
// answered by the planner's CPU executor on the calling thread, without a handle or a device (tools/epipolar_bench.py,
// tests/test_epipolar_capi.py).
int sg_slam_debug_epipolar_timing(sg_slam* s, int32_t enable) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s, SG_EINVAL, "null handle");
  EpipolarSolverOf(s).SetTiming(enable != 0);
  SG_CAPI_END
}

int sg_slam_debug_epipolar_kernel_ms(sg_slam* s, double* ms) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && ms, SG_EINVAL, "null argument");
  *ms = EpipolarSolverOf(s).last_kernel_ms();
  SG_CAPI_END
}

int sg_debug_match_epipolar_cpu(const sg_map* map, const int32_t* pairs, int32_t n, const int32_t* a_offset,
                                const double* a_xy, const uint64_t* a_desc, const int32_t* a_level,
                                const int32_t* b_offset, const double* b_xy, const uint64_t* b_desc,
                                const int32_t* b_level, const sg_epipolar_options* options, int32_t* match,
                                int32_t* best_kp, int32_t* best_dist, int32_t* second_dist, int32_t* num_candidates,
                                sg_epipolar_result* results) {
  SG_CAPI_BEGIN
  SG_REQUIRE(map && options && match, SG_EINVAL, "null argument");
  MatchEpipolar(nullptr, map, pairs, n, a_offset, a_xy, a_desc, a_level, b_offset, b_xy, b_desc, b_level, options,
                match, best_kp, best_dist, second_dist, num_candidates, results);
  SG_CAPI_END
}

static sg::PoseGraphSolver& PoseGraphSolverOf(sg_slam* s) {
  if (!s->posegraph) s->posegraph.reset(new sg::PoseGraphSolver(s->dev, s->solver->stream()));   // one stream per Slam object
  return *s->posegraph;
}

int sg_slam_optimize_pose_graph(sg_slam* s, sg_map* map, const int32_t* node_frame, const int32_t* node_fixed,
                                const int32_t* node_offset, const int32_t* edge_ab, const double* edge_meas,
                                const double* edge_weight, const int32_t* edge_offset, int32_t n,
                                const sg_posegraph_options* options, int32_t* status, double* log_scale,
                                sg_solver_summary* summaries) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && options, SG_EINVAL, "null argument");
  sg::PgPlan plan;
  sg::PlanPoseGraph(map, node_frame, node_fixed, node_offset, edge_ab, edge_meas, edge_weight, edge_offset, n, options,
                    &plan);   // every argument check, on the host
  if (n == 0) return SG_OK;   // nothing to optimise: neither the handle nor the device is touched
  SG_REQUIRE(status, SG_EINVAL, "null status array");
  if (plan.num_run == 0) {   // every status was decided on the host: the device is not touched
    for (int g = 0; g < n; ++g) status[g] = plan.graphs[g].status;
    for (int i = 0; log_scale && i < node_offset[n]; ++i) log_scale[i] = 0.0;
    sg_solver_summary none{};
    none.termination_type = SG_DID_NOT_RUN;
    for (int g = 0; summaries && g < n; ++g) summaries[g] = none;
    return SG_OK;
  }
  sg::PoseGraphSolver& ps = PoseGraphSolverOf(s);
  ps.Solve(map, plan, *options, s->options, status, log_scale, summaries);
  // Slam::Run's bookkeeping (slam.cpp:517-518) over the graphs that ran, in list order
  for (const sg_solver_summary& sum : ps.summaries()) {
    if (sum.termination_type == SG_DID_NOT_RUN) continue;
    s->iterations += sum.num_iterations;
    s->error = sum.final_cost;
    s->last = sum;
  }
  SG_CAPI_END
}

// Diagnostics (not in the public header): HIP-event time of the k_posegraph_lm launch, and the same call solved by
// the planner's CPU executor on the host, no handle and no device (tools/posegraph_bench.py's baseline, and the
// CPU tests' check of the plan and the arithmetic the kernel shares).
int sg_slam_debug_posegraph_timing(sg_slam* s, int32_t enable) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s, SG_EINVAL, "null handle");
  PoseGraphSolverOf(s).SetTiming(enable != 0);
  SG_CAPI_END
}

int sg_slam_debug_posegraph_kernel_ms(sg_slam* s, double* ms) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && ms, SG_EINVAL, "null argument");
  *ms = PoseGraphSolverOf(s).last_kernel_ms();
  SG_CAPI_END
}

int sg_posegraph_debug_cpu_solve(sg_map* map, const int32_t* node_frame, const int32_t* node_fixed,
                                 const int32_t* node_offset, const int32_t* edge_ab, const double* edge_meas,
                                 const double* edge_weight, const int32_t* edge_offset, int32_t n,
                                 const sg_posegraph_options* options, const sg_solver_options* solver, int32_t* status,
                                 double* log_scale, sg_solver_summary* summaries) {
  SG_CAPI_BEGIN
  SG_REQUIRE(map && options && solver, SG_EINVAL, "null argument");
  sg::PgPlan plan;
  sg::PlanPoseGraph(map, node_frame, node_fixed, node_offset, edge_ab, edge_meas, edge_weight, edge_offset, n, options,
                    &plan);
  if (n == 0) return SG_OK;
  SG_REQUIRE(status, SG_EINVAL, "null status array");
  std::vector<double> ws(plan.WorkspaceDoubles(), 0.0), xres(plan.x0);
  const sg::PgView v = plan.View(ws.data());
  sg_solver_summary none{};
  none.termination_type = SG_DID_NOT_RUN;
  std::vector<sg_solver_summary> sums((size_t)n, none);
  for (int g = 0; g < n; ++g) {
    const sg::PgGraph& G = plan.graphs[g];
    status[g] = G.status;
    if (!G.run) continue;
    sg::PgOut out{};
    sg::PgCpuSolve(v, G, *solver, &out);
    sg::PgSummarize(out, &sums[g]);
    if (!out.ok) status[g] = SG_PG_FAILED;
    std::copy(v.x[out.cur] + sg::kPgState * (size_t)G.node0, v.x[out.cur] + sg::kPgState * (size_t)(G.node0 + G.nn),
              xres.begin() + sg::kPgState * (size_t)G.node0);
  }
  sg::PgWriteBack(map, plan, status, xres.data(), options->move_points, log_scale);
  for (int g = 0; summaries && g < n; ++g) summaries[g] = sums[g];
  SG_CAPI_END
}

static sg::PointSolver& PointSolverOf(sg_slam* s) {
  if (!s->points) s->points.reset(new sg::PointSolver(s->dev, s->solver->stream()));   // one stream per Slam object
  return *s->points;
}

int sg_slam_solve_points(sg_slam* s, sg_map* map, const int32_t* points, int32_t n, double range, int32_t* solved,
                         sg_solver_summary* summaries) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map, SG_EINVAL, "null argument");
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative point count");
  if (n == 0) return SG_OK;   // nothing to solve: neither the handle nor the device is touched
  SG_REQUIRE(points && solved, SG_EINVAL, "null point list or result array");
  sg::PointSolver& ps = PointSolverOf(s);
  ps.Solve(map, points, n, range, s->options, solved, summaries);
  // Slam::Run's bookkeeping (slam.cpp:517-518) over the points that ran, in list order
  for (const sg_solver_summary& sum : ps.summaries()) {
    if (sum.termination_type == SG_DID_NOT_RUN) continue;
    s->iterations += sum.num_iterations;
    s->error = sum.final_cost;
    s->last = sum;
  }
  SG_CAPI_END
}

int sg_slam_triangulate_points(sg_slam* s, sg_map* map, const int32_t* points, int32_t n,
                               const sg_triangulate_options* options, int32_t* solved,
                               sg_triangulate_result* results, sg_solver_summary* summaries) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && map && options, SG_EINVAL, "null argument");
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative point count");
  if (n == 0) return SG_OK;   // nothing to triangulate: neither the handle nor the device is touched
  SG_REQUIRE(points && solved, SG_EINVAL, "null point list or result array");
  sg::PointSolver& ps = PointSolverOf(s);
  ps.Triangulate(map, points, n, *options, s->options, solved, results, summaries);
  // Slam::Run's bookkeeping (slam.cpp:517-518) over the points the polish ran on, in list order
  for (const sg_solver_summary& sum : ps.summaries()) {
    if (sum.termination_type == SG_DID_NOT_RUN) continue;
    s->iterations += sum.num_iterations;
    s->error = sum.final_cost;
    s->last = sum;
  }
  SG_CAPI_END
}

// Diagnostics (not in the public header): HIP-event time of the k_point_lm launch (tools/points_bench.py); after
// sg_slam_triangulate_points, of its one or two launches (tools/triangulate_bench.py).
int sg_slam_debug_points_timing(sg_slam* s, int32_t enable) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s, SG_EINVAL, "null handle");
  PointSolverOf(s).SetTiming(enable != 0);
  SG_CAPI_END
}

int sg_slam_debug_points_kernel_ms(sg_slam* s, double* ms) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && ms, SG_EINVAL, "null argument");
  *ms = PointSolverOf(s).last_kernel_ms();
  SG_CAPI_END
}

int32_t sg_slam_iterations(const sg_slam* s) { return s ? s->iterations : 0; }
double sg_slam_error(const sg_slam* s) { return s ? s->error : 0.0; }

int sg_slam_load_counts(const sg_slam* s, int32_t* full_loads, int32_t* value_loads) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && full_loads && value_loads, SG_EINVAL, "null argument");
  *full_loads = *value_loads = 0;
  if (s->solver) s->solver->LoadCounts(full_loads, value_loads);
  SG_CAPI_END
}

int sg_slam_last_summary(const sg_slam* s, sg_solver_summary* out) {
  SG_CAPI_BEGIN
  SG_REQUIRE(s && out, SG_EINVAL, "null argument");
  *out = s->last;
  SG_CAPI_END
}

}  // extern "C"
