// problem.cpp — host side of the drop-in boundary: LocalMap SoA -> compact BA problem.
//
// Implements the frame / point selection rules of Slam::SolveFrames (slam.cpp:417-443),
// Slam::SolveAllFrames (slam.cpp:447-480) and Slam::SetupProblem (slam.cpp:257-414) on the sg_map view of
// a LocalMap, producing the sg_problem the device solver consumes.  Ceres keeps pointers into the map;
// here the solved blocks are copied back by sg_problem_write_back (same observable effect).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "common.h"

namespace sg {

static thread_local std::string g_last_error;
void SetError(const std::string& msg) { g_last_error = msg; }

namespace {

struct ProblemStorage {
  std::vector<double> k, q, t, X, obs_pt;
  std::vector<int32_t> frame_camera, frame_map_index, point_map_index, obs_frame, obs_point, dist_frame,
      dist_prev;
  std::vector<uint8_t> frame_rot_free, frame_trans_free, point_free;

  void Clear() {
    for (auto* v : {&k, &q, &t, &X, &obs_pt}) v->clear();
    for (auto* v : {&frame_camera, &frame_map_index, &point_map_index, &obs_frame, &obs_point, &dist_frame, &dist_prev})
      v->clear();
    for (auto* v : {&frame_rot_free, &frame_trans_free, &point_free}) v->clear();
  }

  void Bind(sg_problem* p) {
    p->k = k.data();
    p->q = q.data();
    p->t = t.data();
    p->frame_camera = frame_camera.data();
    p->frame_rot_free = frame_rot_free.data();
    p->frame_trans_free = frame_trans_free.data();
    p->frame_map_index = frame_map_index.data();
    p->X = X.data();
    p->point_free = point_free.data();
    p->point_map_index = point_map_index.data();
    p->obs_pt = obs_pt.data();
    p->obs_frame = obs_frame.data();
    p->obs_point = obs_point.data();
    p->dist_frame = dist_frame.data();
    p->dist_prev = dist_prev.data();
    p->num_frames = (int32_t)frame_camera.size();
    p->num_points = (int32_t)point_free.size();
    p->num_obs = (int32_t)obs_frame.size();
    p->num_dist = (int32_t)dist_frame.size();
    p->num_cameras = (int32_t)(k.size() / 7);
    p->owner_ = this;
  }
};

// A freed problem's storage is kept for the thread's next problem (main.cpp builds one per SolveFrames call,
// each about the size of the last): its vectors keep their capacity, so a build neither allocates nor
// page-faults.  Build's scratch arrays are kept the same way.
constexpr size_t kStoragePool = 2;
thread_local std::vector<std::unique_ptr<ProblemStorage>> t_pool;

ProblemStorage* TakeStorage() {
  if (t_pool.empty()) return new ProblemStorage;
  ProblemStorage* st = t_pool.back().release();
  t_pool.pop_back();
  st->Clear();
  return st;
}

void ReturnStorage(ProblemStorage* st) {
  if (t_pool.size() < kStoragePool)
    t_pool.emplace_back(st);
  else
    delete st;
}

struct BuildScratch {
  std::vector<uint8_t> frame_used, point_in, point_fluid;
  std::vector<int32_t> obs_in, point_index, pts, frame_index;
};
thread_local BuildScratch t_scratch;

constexpr int kUnusableMask = (1 << SG_BAD_LOCATION) | (1 << SG_NO_BASELINE) | (1 << SG_NO_OBSERVATIONS) |
                              (1 << SG_BAD_FEATURE);  // TrackedPoint::slam_usable, localmap.h:242-248

// Validates the map; returns whether its observations are ordered by frame (a LocalMap's are: each frame's
// observations are appended when the frame is tracked), which lets Build walk only the presented frames' range.
bool CheckMap(const sg_map* m) {
  SG_REQUIRE(m != nullptr, SG_EINVAL, "null map");
  SG_REQUIRE(m->num_frames >= 0 && m->num_points >= 0 && m->num_obs >= 0 && m->num_cameras >= 0, SG_EINVAL,
             "negative map sizes");
  for (int32_t f = 0; f < m->num_frames; ++f) {
    SG_REQUIRE(m->frame_camera[f] >= 0 && m->frame_camera[f] < m->num_cameras, SG_EINVAL,
               "frame_camera out of range");
    SG_REQUIRE(m->frame_prev[f] >= -1 && m->frame_prev[f] < m->num_frames, SG_EINVAL, "frame_prev out of range");
  }
  // one branch-free sweep (the range tests and the order test accumulate), then the failing index if any
  const uint32_t F = (uint32_t)m->num_frames, P = (uint32_t)m->num_points;
  bool bad = false, sorted = true;
  int32_t prev = 0;
  for (int32_t o = 0; o < m->num_obs; ++o) {
    const int32_t f = m->obs_frame[o];
    bad |= ((uint32_t)f >= F) | ((uint32_t)m->obs_point[o] >= P);
    sorted &= f >= prev;
    prev = f;
  }
  if (bad)
    for (int32_t o = 0; o < m->num_obs; ++o) {
      SG_REQUIRE(m->obs_frame[o] >= 0 && m->obs_frame[o] < m->num_frames, SG_EINVAL, "obs_frame out of range");
      SG_REQUIRE(m->obs_point[o] >= 0 && m->obs_point[o] < m->num_points, SG_EINVAL, "obs_point out of range");
    }
  return sorted;
}

// role[f]: 0 = not presented, 1 = presented & solved, 2 = presented & constant.
bool Build(const sg_map* m, const std::vector<uint8_t>& role, double range, bool cameras_free, bool obs_by_frame,
           sg_problem* out) {
  const int F = m->num_frames, P = m->num_points, M = m->num_obs;
  // Observations to visit: all of them, or (observations ordered by frame) the range of the presented frames.
  int o_lo = 0, o_hi = M;
  if (obs_by_frame) {
    int fmin = F, fmax = -1;
    for (int f = 0; f < F; ++f)
      if (role[f]) {
        fmin = std::min(fmin, f);
        fmax = std::max(fmax, f);
      }
    o_lo = (int)(std::lower_bound(m->obs_frame, m->obs_frame + M, fmin) - m->obs_frame);
    o_hi = (int)(std::upper_bound(m->obs_frame + o_lo, m->obs_frame + M, fmax) - m->obs_frame);
  }
  // Pass 1 (slam.cpp:274-303): usable observations of presented frames, in map order (branch-free: the
  // selection is data-dependent, so the marks are or-ed in and the list is compacted by its running count).
  BuildScratch& sc = t_scratch;
  std::vector<uint8_t>&frame_used = sc.frame_used, &point_in = sc.point_in, &point_fluid = sc.point_fluid;
  frame_used.assign(F, 0);
  point_in.assign(P, 0);
  point_fluid.assign(P, 0);
  std::vector<int32_t>& obs_in = sc.obs_in;
  obs_in.resize(std::max(o_hi - o_lo, 0));
  size_t nin = 0;
  for (int o = o_lo; o < o_hi; ++o) {
    const int f = m->obs_frame[o], pt = m->obs_point[o];
    const uint8_t use = (role[f] != 0) & (m->obs_disabled[o] == 0) & ((m->point_flags[pt] & kUnusableMask) == 0);
    obs_in[nin] = o;
    nin += use;
    frame_used[f] |= use;
    point_in[pt] |= use;
    point_fluid[pt] |= use & (role[f] == 1);
  }
  int used = 0;
  for (int f = 0; f < F; ++f) {
    used += role[f] != 0 && frame_used[f];
  }
  if (used < 2) return false;  // "Slam aborted due to frame set too small" (slam.cpp:305-308)

  auto* st = TakeStorage();
  std::vector<int32_t>& frame_index = sc.frame_index;
  frame_index.assign(F, -1);
  auto add_frame = [&](int f, bool rot_free, bool trans_free) {
    frame_index[f] = (int32_t)st->frame_camera.size();
    st->frame_camera.push_back(m->frame_camera[f]);
    st->frame_map_index.push_back(f);
    st->frame_rot_free.push_back(rot_free);
    st->frame_trans_free.push_back(trans_free);
    st->q.insert(st->q.end(), m->q + 4 * f, m->q + 4 * f + 4);
    st->t.insert(st->t.end(), m->t + 3 * f, m->t + 3 * f + 3);
  };
  // Used frames become quaternion + translation blocks, constant when not solved (slam.cpp:314-333).
  for (int f = 0; f < F; ++f)
    if (role[f] && frame_used[f]) add_frame(f, role[f] == 1, role[f] == 1);
  // FrameDistance between every solved, used frame and its presented previous frame (slam.cpp:383-411).
  // A presented but unused previous frame contributes a fresh (free) translation block.
  for (int f = 0; f < F; ++f) {
    if (role[f] != 1 || !frame_used[f]) continue;
    const int prev = m->frame_prev[f];
    if (prev < 0 || !role[prev]) continue;
    if (frame_index[prev] < 0) add_frame(prev, false, true);
    st->dist_frame.push_back(frame_index[f]);
    st->dist_prev.push_back(frame_index[prev]);
  }
  // Points (slam.cpp:345-354).
  std::vector<int32_t>&point_index = sc.point_index, &pts = sc.pts;
  point_index.assign(P, -1);
  pts.resize(P);
  size_t npt = 0;
  for (int pt = 0; pt < P; ++pt) {   // compaction of the marked points, in map order
    pts[npt] = pt;
    npt += point_in[pt];
  }
  st->point_map_index.assign(pts.begin(), pts.begin() + npt);
  st->point_free.resize(npt);
  st->X.resize(4 * npt);
  for (size_t i = 0; i < npt; ++i) {
    const int pt = pts[i];
    point_index[pt] = (int32_t)i;
    const bool is_const = m->point_uncertainty[pt] <= 100.0 && !point_fluid[pt];
    st->point_free[i] = !is_const;
    std::memcpy(st->X.data() + 4 * i, m->X + 4 * (size_t)pt, 4 * sizeof(double));
  }
  st->obs_pt.resize(2 * nin);
  st->obs_frame.resize(nin);
  st->obs_point.resize(nin);
  for (size_t i = 0; i < nin; ++i) {
    const int o = obs_in[i];
    st->obs_pt[2 * i] = m->obs_pt[2 * o];
    st->obs_pt[2 * i + 1] = m->obs_pt[2 * o + 1];
    st->obs_frame[i] = frame_index[m->obs_frame[o]];
    st->obs_point[i] = point_index[m->obs_point[o]];
  }
  st->k.assign(m->k, m->k + 7 * m->num_cameras);
  std::memset(out, 0, sizeof(*out));
  st->Bind(out);
  out->cameras_free = cameras_free ? 1 : 0;
  out->range = range;
  out->dist_target = 150.0;  // slam.cpp:403
  out->dist_range = 15.0;    // slam.cpp:404
  out->stab_range = 5.0;     // slam.cpp:463
  return true;
}

void CheckProblem(const sg_problem* p) {
  SG_REQUIRE(p != nullptr, SG_EINVAL, "null problem");
  for (int32_t o = 0; o < p->num_obs; ++o) {
    SG_REQUIRE(p->obs_frame[o] >= 0 && p->obs_frame[o] < p->num_frames, SG_EINVAL, "obs_frame out of range");
    SG_REQUIRE(p->obs_point[o] >= 0 && p->obs_point[o] < p->num_points, SG_EINVAL, "obs_point out of range");
  }
  for (int32_t d = 0; d < p->num_dist; ++d)
    SG_REQUIRE(p->dist_frame[d] >= 0 && p->dist_frame[d] < p->num_frames && p->dist_prev[d] >= 0 &&
                   p->dist_prev[d] < p->num_frames,
               SG_EINVAL, "FrameDistance frame out of range");
  for (int32_t f = 0; f < p->num_frames; ++f)
    SG_REQUIRE(p->frame_camera[f] >= 0 && p->frame_camera[f] < p->num_cameras, SG_EINVAL,
               "frame_camera out of range");
}

}  // namespace

void ValidateProblem(const sg_problem* p) { CheckProblem(p); }

}  // namespace sg

extern "C" {

const char* sg_version(void) { return "slamgpu 0.1 (gfx950)"; }
const char* sg_last_error(void) { return sg::g_last_error.c_str(); }

void sg_solver_options_default(sg_solver_options* o) {
  o->max_num_iterations = 1000;     // slam.cpp:493
  o->function_tolerance = 1e-7;     // slam.cpp:494
  o->gradient_tolerance = 1e-10;    // Ceres 1.8 defaults below
  o->parameter_tolerance = 1e-8;
  o->min_relative_decrease = 1e-3;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
  o->disable_termination = 0;
  o->always_linearize = 0;
}

void sg_triangulate_options_default(sg_triangulate_options* o) {
  o->min_parallax = 0.0;   // gates off
  o->max_error_px = 0.0;
  o->refine = 0;
  o->range = 2.0;          // main.cpp's CauchyLoss range
}

void sg_localize_options_default(sg_localize_options* o) {
  o->threshold_px = 4.0;
  o->max_hypotheses = 1024;
  o->min_inliers = 8;
  o->seed = 0;
  o->refine = 1;
  o->range = 2.0;          // main.cpp's CauchyLoss range
}

void sg_relpose_options_default(sg_relpose_options* o) {
  o->threshold_px = 2.0;
  o->max_hypotheses = 1024;
  o->min_inliers = 16;
  o->min_parallax = 0.0;
  o->seed = 0;
  o->refine = 1;
  o->baseline = 0.0;
}

void sg_align_options_default(sg_align_options* o) {
  o->threshold = 10.0;
  o->max_hypotheses = 1024;
  o->min_inliers = 8;
  o->seed = 0;
  o->refine = 1;
  o->fix_scale = 0;
  o->max_scale = 0.0;      // no gate
  o->min_gap = 1e-6;
}

void sg_match_options_default(sg_match_options* o) {
  o->radius_px = 12.0;
  o->width = 0;   // no image bound
  o->height = 0;
  o->max_dist = 64;
  o->ratio_percent = 80;
  o->skip_observed = 1;
}

void sg_epipolar_options_default(sg_epipolar_options* o) {
  o->tol_px = 2.0;
  o->min_parallax = 0.0;   // no parallax test
  o->max_dist = 64;
  o->ratio_percent = 80;
}

int sg_map_apply_similarity(sg_map* map, double scale, const double* q, const double* t, const int32_t* frames,
                            int32_t nf, const int32_t* points, int32_t np) {
  SG_CAPI_BEGIN
  SG_REQUIRE(map && q && t, SG_EINVAL, "null argument");
  SG_REQUIRE(nf >= 0 && np >= 0, SG_EINVAL, "negative count");
  SG_REQUIRE((nf == 0 || frames) && (np == 0 || points), SG_EINVAL, "null index list");
  SG_REQUIRE(std::isfinite(scale) && scale > 0.0, SG_EINVAL, "scale must be positive and finite");
  const double n2 = (q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]);
  SG_REQUIRE(std::fabs(n2 - 1.0) <= 1e-9, SG_EINVAL, "q is not a unit quaternion");   // (false for NaN)
  SG_REQUIRE(std::isfinite(t[0]) && std::isfinite(t[1]) && std::isfinite(t[2]), SG_EINVAL, "t is not finite");
  SG_REQUIRE(map->num_frames >= 0 && map->num_points >= 0, SG_EINVAL, "negative map sizes");
  SG_REQUIRE((nf == 0 || (map->q && map->t)) && (np == 0 || map->X), SG_EINVAL, "the map's arrays cannot be read");
  std::vector<uint8_t> seen_f((size_t)map->num_frames, 0), seen_p((size_t)map->num_points, 0);
  for (int i = 0; i < nf; ++i) {
    SG_REQUIRE(frames[i] >= 0 && frames[i] < map->num_frames, SG_EINVAL, "frame index out of range");
    SG_REQUIRE(!seen_f[frames[i]], SG_EINVAL, "frame listed twice");
    seen_f[frames[i]] = 1;
  }
  for (int i = 0; i < np; ++i) {
    SG_REQUIRE(points[i] >= 0 && points[i] < map->num_points, SG_EINVAL, "point index out of range");
    SG_REQUIRE(!seen_p[points[i]], SG_EINVAL, "point listed twice");
    seen_p[points[i]] = 1;
  }
  // A = scale R(q), q normalised; R the standard matrix of a unit quaternion in Eigen memory [x, y, z, w]
  const double in = 1.0 / std::sqrt(n2);
  const double x = q[0] * in, y = q[1] * in, z = q[2] * in, w = q[3] * in;
  const double A[9] = {scale * (1.0 - 2.0 * (y * y + z * z)), scale * (2.0 * (x * y - w * z)),
                       scale * (2.0 * (x * z + w * y)),       scale * (2.0 * (x * y + w * z)),
                       scale * (1.0 - 2.0 * (x * x + z * z)), scale * (2.0 * (y * z - w * x)),
                       scale * (2.0 * (x * z - w * y)),       scale * (2.0 * (y * z + w * x)),
                       scale * (1.0 - 2.0 * (x * x + y * y))};
  for (int i = 0; i < np; ++i) {
    double* X = map->X + 4 * (size_t)points[i];
    const double v[3] = {X[0], X[1], X[2]};
    for (int r = 0; r < 3; ++r) X[r] = (A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2]) + t[r] * X[3];
  }
  for (int i = 0; i < nf; ++i) {
    double* tf = map->t + 3 * (size_t)frames[i];
    double* qf = map->q + 4 * (size_t)frames[i];
    const double v[3] = {tf[0], tf[1], tf[2]};
    for (int r = 0; r < 3; ++r) tf[r] = (A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2]) + t[r];
    // q_f (x) conj(q): the rotation of conj(q), then that of q_f
    const double p[4] = {qf[0], qf[1], qf[2], qf[3]}, c[4] = {-x, -y, -z, w};
    double r4[4] = {p[3] * c[0] + p[0] * c[3] + p[1] * c[2] - p[2] * c[1],
                    p[3] * c[1] - p[0] * c[2] + p[1] * c[3] + p[2] * c[0],
                    p[3] * c[2] + p[0] * c[1] - p[1] * c[0] + p[2] * c[3],
                    p[3] * c[3] - p[0] * c[0] - p[1] * c[1] - p[2] * c[2]};
    double rn = 1.0 / std::sqrt((r4[0] * r4[0] + r4[1] * r4[1]) + (r4[2] * r4[2] + r4[3] * r4[3]));
    if (r4[3] < 0.0) rn = -rn;
    for (int k = 0; k < 4; ++k) qf[k] = r4[k] * rn;
  }
  SG_CAPI_END
}

void sg_posegraph_options_default(sg_posegraph_options* o) {
  o->range = 0.0;          // no loss
  o->fix_scale = 0;
  o->move_points = 0;
}

int sg_map_pose_edges(const sg_map* map, const int32_t* pairs, int32_t n, const double* sim, double* meas) {
  SG_CAPI_BEGIN
  SG_REQUIRE(map, SG_EINVAL, "null map");
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative count");
  SG_REQUIRE(n == 0 || (pairs && meas), SG_EINVAL, "null pair list or output");
  SG_REQUIRE(map->num_frames >= 0, SG_EINVAL, "negative map sizes");
  SG_REQUIRE(n == 0 || (map->q && map->t), SG_EINVAL, "the map's poses cannot be read");
  double s = 1.0, qs[4] = {0.0, 0.0, 0.0, 1.0}, ts[3] = {0.0, 0.0, 0.0};
  if (sim) {
    s = sim[0];
    SG_REQUIRE(std::isfinite(s) && s > 0.0, SG_EINVAL, "scale must be positive and finite");
    const double n2 = (sim[1] * sim[1] + sim[2] * sim[2]) + (sim[3] * sim[3] + sim[4] * sim[4]);
    SG_REQUIRE(std::fabs(n2 - 1.0) <= 1e-9, SG_EINVAL, "q is not a unit quaternion");   // (false for NaN)
    SG_REQUIRE(std::isfinite(sim[5]) && std::isfinite(sim[6]) && std::isfinite(sim[7]), SG_EINVAL, "t is not finite");
    const double in = 1.0 / std::sqrt(n2);
    for (int k = 0; k < 4; ++k) qs[k] = sim[1 + k] * in;
    for (int k = 0; k < 3; ++k) ts[k] = sim[5 + k];
  }
  for (int i = 0; i < n; ++i) {
    const int a = pairs[2 * (size_t)i], b = pairs[2 * (size_t)i + 1];
    SG_REQUIRE(a >= 0 && a < map->num_frames && b >= 0 && b < map->num_frames, SG_EINVAL, "frame index out of range");
    SG_REQUIRE(a != b, SG_EINVAL, "a pair of one frame");
  }
  // Hamilton product on Eigen memory, and p = R(q) d by the standard matrix of a unit quaternion
  const auto mul = [](const double* p, const double* c, double* r) {
    r[0] = p[3] * c[0] + p[0] * c[3] + p[1] * c[2] - p[2] * c[1];
    r[1] = p[3] * c[1] - p[0] * c[2] + p[1] * c[3] + p[2] * c[0];
    r[2] = p[3] * c[2] + p[0] * c[1] - p[1] * c[0] + p[2] * c[3];
    r[3] = p[3] * c[3] - p[0] * c[0] - p[1] * c[1] - p[2] * c[2];
  };
  const auto unit = [](double* q) {
    double rn = 1.0 / std::sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    if (q[3] < 0.0) rn = -rn;
    for (int k = 0; k < 4; ++k) q[k] *= rn;
  };
  const auto rot = [](const double* q, const double* d, double* p) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    p[0] = (1.0 - 2.0 * (y * y + z * z)) * d[0] + 2.0 * (x * y - w * z) * d[1] + 2.0 * (x * z + w * y) * d[2];
    p[1] = 2.0 * (x * y + w * z) * d[0] + (1.0 - 2.0 * (x * x + z * z)) * d[1] + 2.0 * (y * z - w * x) * d[2];
    p[2] = 2.0 * (x * z - w * y) * d[0] + 2.0 * (y * z + w * x) * d[1] + (1.0 - 2.0 * (x * x + y * y)) * d[2];
  };
  const double cs[4] = {-qs[0], -qs[1], -qs[2], qs[3]};
  for (int i = 0; i < n; ++i) {
    const int a = pairs[2 * (size_t)i], b = pairs[2 * (size_t)i + 1];
    const double* qb = map->q + 4 * (size_t)b;
    const double* tb = map->t + 3 * (size_t)b;
    double qa[4], ta[3];
    for (int k = 0; k < 4; ++k) qa[k] = map->q[4 * (size_t)a + k];
    for (int k = 0; k < 3; ++k) ta[k] = map->t[3 * (size_t)a + k];
    if (sim) {   // frame a as sg_map_apply_similarity would leave it
      double r4[4], rt[3];
      mul(qa, cs, r4);
      unit(r4);
      rot(qs, ta, rt);
      for (int k = 0; k < 4; ++k) qa[k] = r4[k];
      for (int k = 0; k < 3; ++k) ta[k] = s * rt[k] + ts[k];
    }
    double* o = meas + 8 * (size_t)i;
    const double cb[4] = {-qb[0], -qb[1], -qb[2], qb[3]};
    mul(qa, cb, o);
    unit(o);
    double qu[4] = {qa[0], qa[1], qa[2], qa[3]};
    unit(qu);
    const double d[3] = {tb[0] - ta[0], tb[1] - ta[1], tb[2] - ta[2]};
    rot(qu, d, o + 4);
    for (int k = 0; k < 3; ++k) o[4 + k] /= s;
    o[7] = sim ? -std::log(s) : 0.0;
  }
  SG_CAPI_END
}

int sg_map_covisible_pairs(const sg_map* map, const int32_t* frames, int32_t nf, int32_t min_shared,
                           int32_t* pairs_out, int32_t cap, int32_t* count) {
  SG_CAPI_BEGIN
  SG_REQUIRE(map && count, SG_EINVAL, "null argument");
  SG_REQUIRE(nf >= 0 && cap >= 0 && min_shared >= 1, SG_EINVAL, "bad count");
  SG_REQUIRE((nf == 0 || frames) && (cap == 0 || pairs_out), SG_EINVAL, "null list");
  SG_REQUIRE(map->num_frames >= 0 && map->num_points >= 0 && map->num_obs >= 0, SG_EINVAL, "negative map sizes");
  SG_REQUIRE(map->num_obs == 0 || (map->obs_frame && map->obs_point && map->obs_disabled && map->point_flags),
             SG_EINVAL, "the map's observations cannot be read");
  std::vector<int32_t> pos((size_t)map->num_frames, -1);
  for (int i = 0; i < nf; ++i) {
    SG_REQUIRE(frames[i] >= 0 && frames[i] < map->num_frames, SG_EINVAL, "frame index out of range");
    SG_REQUIRE(pos[frames[i]] < 0, SG_EINVAL, "frame listed twice");
    pos[frames[i]] = i;
  }
  // per point, the list positions that see it through an enabled observation (each once)
  std::vector<std::vector<int32_t>> seen_by((size_t)map->num_points);
  for (int o = 0; o < map->num_obs; ++o) {
    const int f = map->obs_frame[o], p = map->obs_point[o];
    SG_REQUIRE(f >= 0 && f < map->num_frames && p >= 0 && p < map->num_points, SG_EINVAL,
               "observation index out of range");
    if (map->obs_disabled[o] || pos[f] < 0 || (map->point_flags[p] & sg::kUnusableMask) != 0) continue;
    std::vector<int32_t>& v = seen_by[p];
    if (std::find(v.begin(), v.end(), pos[f]) == v.end()) v.push_back(pos[f]);
  }
  std::vector<int32_t> shared((size_t)nf * nf, 0);
  for (const std::vector<int32_t>& v : seen_by)
    for (size_t i = 0; i < v.size(); ++i)
      for (size_t j = i + 1; j < v.size(); ++j)
        shared[(size_t)std::min(v[i], v[j]) * nf + std::max(v[i], v[j])] += 1;
  int32_t c = 0;
  for (int i = 0; i < nf; ++i)
    for (int j = i + 1; j < nf; ++j) {
      if (shared[(size_t)i * nf + j] < min_shared) continue;
      if (c < cap) {
        pairs_out[2 * (size_t)c] = i;
        pairs_out[2 * (size_t)c + 1] = j;
      }
      c += 1;
    }
  *count = c;
  SG_CAPI_END
}

void sg_device_options_default(sg_device_options* o) {
  o->device = 0;
  o->precision = 0;
  o->rank = 0;
  o->nranks = 1;
}

int sg_problem_from_map_frames(const sg_map* map, int32_t num_to_solve, int32_t num_to_present, double range,
                               sg_problem* out, int32_t* built) {
  SG_CAPI_BEGIN
  const bool obs_by_frame = sg::CheckMap(map);
  SG_REQUIRE(out && built, SG_EINVAL, "null output");
  // slam.cpp:423-434: the newest num_to_solve frames are solved, the next ones up to num_to_present are
  // presented as constant.
  std::vector<uint8_t> role(map->num_frames, 0);
  for (int i = 0; i < map->num_frames; ++i) {
    const int f = map->num_frames - i - 1;
    if (i < num_to_solve) role[f] = 1;
    else if (i < num_to_present) role[f] = 2;
    else break;
  }
  *built = sg::Build(map, role, range, false, obs_by_frame, out) ? 1 : 0;
  SG_CAPI_END
}

int sg_problem_from_map_all(const sg_map* map, double range, int32_t solve_cameras, sg_problem* out,
                            int32_t* built) {
  SG_CAPI_BEGIN
  const bool obs_by_frame = sg::CheckMap(map);
  SG_REQUIRE(out && built, SG_EINVAL, "null output");
  std::vector<uint8_t> role(map->num_frames, 1);  // slam.cpp:449-452
  *built = sg::Build(map, role, range, solve_cameras != 0, obs_by_frame, out) ? 1 : 0;
  SG_CAPI_END
}

void sg_problem_free(sg_problem* p) {
  if (p && p->owner_) {
    sg::ReturnStorage(static_cast<sg::ProblemStorage*>(p->owner_));
    p->owner_ = nullptr;
  }
}

int sg_problem_write_back(const sg_problem* p, sg_map* map) {
  SG_CAPI_BEGIN
  SG_REQUIRE(p && map, SG_EINVAL, "null argument");
  for (int32_t f = 0; f < p->num_frames; ++f) {
    const int32_t mf = p->frame_map_index[f];
    SG_REQUIRE(mf >= 0 && mf < map->num_frames, SG_EINVAL, "frame_map_index out of range");
    std::memcpy(map->q + 4 * mf, p->q + 4 * f, 4 * sizeof(double));
    std::memcpy(map->t + 3 * mf, p->t + 3 * f, 3 * sizeof(double));
  }
  for (int32_t i = 0; i < p->num_points; ++i) {
    const int32_t mp = p->point_map_index[i];
    SG_REQUIRE(mp >= 0 && mp < map->num_points, SG_EINVAL, "point_map_index out of range");
    std::memcpy(map->X + 4 * mp, p->X + 4 * i, 4 * sizeof(double));
  }
  if (p->cameras_free) std::memcpy(map->k, p->k, 7 * sizeof(double) * map->num_cameras);
  SG_CAPI_END
}

// Landmark shard: points ordered by their first observing frame, split into nranks contiguous ranges of
// roughly equal observation count; each shard keeps every frame, camera and FrameDistance block.
int sg_problem_shard(const sg_problem* p, int32_t rank, int32_t nranks, sg_problem* out) {
  SG_CAPI_BEGIN
  sg::CheckProblem(p);
  SG_REQUIRE(out && nranks >= 1 && rank >= 0 && rank < nranks, SG_EINVAL, "bad shard arguments");
  const int P = p->num_points, M = p->num_obs;
  std::vector<int32_t> first(P, INT32_MAX), nobs(P, 0);
  for (int o = 0; o < M; ++o) {
    first[p->obs_point[o]] = std::min(first[p->obs_point[o]], p->obs_frame[o]);
    nobs[p->obs_point[o]]++;
  }
  std::vector<int32_t> order(P);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return first[a] < first[b]; });
  // Balanced split on observation counts.
  std::vector<int32_t> owner(P, 0);
  long long total = 0;
  for (int i = 0; i < P; ++i) total += nobs[i];
  long long acc = 0;
  for (int i = 0; i < P; ++i) {
    const int pt = order[i];
    int r = total > 0 ? (int)((acc * nranks) / total) : (int)((long long)i * nranks / std::max(P, 1));
    owner[pt] = std::min(r, nranks - 1);
    acc += nobs[pt];
  }
  auto* st = new sg::ProblemStorage;
  st->k.assign(p->k, p->k + 7 * p->num_cameras);
  st->q.assign(p->q, p->q + 4 * p->num_frames);
  st->t.assign(p->t, p->t + 3 * p->num_frames);
  st->frame_camera.assign(p->frame_camera, p->frame_camera + p->num_frames);
  st->frame_rot_free.assign(p->frame_rot_free, p->frame_rot_free + p->num_frames);
  st->frame_trans_free.assign(p->frame_trans_free, p->frame_trans_free + p->num_frames);
  st->frame_map_index.assign(p->frame_map_index, p->frame_map_index + p->num_frames);
  st->dist_frame.assign(p->dist_frame, p->dist_frame + p->num_dist);
  st->dist_prev.assign(p->dist_prev, p->dist_prev + p->num_dist);
  std::vector<int32_t> local(P, -1);
  for (int i = 0; i < P; ++i) {
    const int pt = order[i];
    if (owner[pt] != rank) continue;
    local[pt] = (int32_t)st->point_free.size();
    st->point_free.push_back(p->point_free[pt]);
    st->point_map_index.push_back(p->point_map_index[pt]);
    st->X.insert(st->X.end(), p->X + 4 * pt, p->X + 4 * pt + 4);
  }
  for (int o = 0; o < M; ++o) {
    const int pt = p->obs_point[o];
    if (owner[pt] != rank) continue;
    st->obs_pt.push_back(p->obs_pt[2 * o]);
    st->obs_pt.push_back(p->obs_pt[2 * o + 1]);
    st->obs_frame.push_back(p->obs_frame[o]);
    st->obs_point.push_back(local[pt]);
  }
  std::memset(out, 0, sizeof(*out));
  st->Bind(out);
  out->cameras_free = p->cameras_free;
  out->range = p->range;
  out->dist_target = p->dist_target;
  out->dist_range = p->dist_range;
  out->stab_range = p->stab_range;
  SG_CAPI_END
}

}  // extern "C"
