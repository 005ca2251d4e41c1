// points_plan_check.cpp — CPU check of the structure-only planner (slam-robot_amd/csrc/points_plan.cpp): on
// generated maps (observations in frame-major map order, some disabled, points carrying flags, points with 0, 1 and
// 2 enabled observations, a point observed by every frame) it recomputes by brute force which observations each
// listed point keeps and in which order, the records, the offsets, the frame table, the cameras, the starts and
// the DID_NOT_RUN decisions, and checks that bad point lists and bad maps are rejected.  Built stand-alone with
// -fsanitize=address,undefined by tests/test_points_plan.py.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "points_plan.h"

using namespace sg;

static int g_fail = 0;
static std::string g_case;
#define CHECK(cond)                                                                                        \
  do {                                                                                                     \
    if (!(cond)) {                                                                                         \
      if (++g_fail <= 40) printf("FAIL [%s] %s:%d: %s\n", g_case.c_str(), __FILE__, __LINE__, #cond);      \
    }                                                                                                      \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(s >> 33);
  }
  int range(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }   // inclusive
  double unit() { return next() / 2147483648.0; }
};

struct Map {
  std::vector<double> k, q, t, X, unc, obs_pt, obs_err;
  std::vector<int32_t> frame_camera, frame_prev, flags, obs_frame, obs_point, obs_disabled;
  sg_map view() {
    sg_map m{};
    m.num_cameras = (int32_t)k.size() / 7;
    m.k = k.data();
    m.num_frames = (int32_t)frame_camera.size();
    m.q = q.data();
    m.t = t.data();
    m.frame_camera = frame_camera.data();
    m.frame_prev = frame_prev.data();
    m.num_points = (int32_t)flags.size();
    m.X = X.data();
    m.point_flags = flags.data();
    m.point_uncertainty = unc.data();
    m.num_obs = (int32_t)obs_frame.size();
    m.obs_pt = obs_pt.data();
    m.obs_frame = obs_frame.data();
    m.obs_point = obs_point.data();
    m.obs_disabled = obs_disabled.data();
    m.obs_error = obs_err.data();
    return m;
  }
};

// F frames, P points; frame by frame (a LocalMap's order) every point is observed with probability about 1/3,
// points kEvery .. kTwo by every frame; about a fifth of the observations are disabled (none of kEvery's).
constexpr int kEvery = 5, kNone = 6, kOne = 7, kTwo = 8;
static Map MakeMap(uint64_t seed, int F, int P) {
  Rng r{seed};
  Map m;
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 7; ++i) m.k.push_back(100.0 * c + i + r.unit());
  for (int f = 0; f < F; ++f) {
    for (int i = 0; i < 4; ++i) m.q.push_back(r.unit());
    for (int i = 0; i < 3; ++i) m.t.push_back(1000.0 * r.unit());
    m.frame_camera.push_back((f + 1) & 1);
    m.frame_prev.push_back(f - 1);
  }
  for (int p = 0; p < P; ++p) {
    for (int i = 0; i < 4; ++i) m.X.push_back(r.unit() * 5000.0);
    // every flag occurs (freshly seeded points carry NO_BASELINE | NO_OBSERVATIONS): none is consulted
    m.flags.push_back(p % 3 == 0 ? (1 << SG_NO_BASELINE) | (1 << SG_NO_OBSERVATIONS) : (p % 7 == 0 ? 1 << (p % 5) : 0));
    m.unc.push_back(1.0);
  }
  for (int f = 0; f < F; ++f)
    for (int p = 0; p < P; ++p) {
      if ((p < kEvery || p > kTwo) && r.range(0, 2) != 0) continue;
      m.obs_frame.push_back(f);
      m.obs_point.push_back(p);
      m.obs_pt.push_back(640.0 * r.unit());
      m.obs_pt.push_back(480.0 * r.unit());
      m.obs_disabled.push_back(p != kEvery && r.range(0, 4) == 0);
      m.obs_err.push_back(0.0);
      m.obs_err.push_back(0.0);
    }
  return m;
}

// Leave exactly `want` of point p's observations enabled (the first ones in map order), the rest disabled.
static void ForceEnabled(Map& m, int p, int want) {
  int have = 0;
  for (size_t o = 0; o < m.obs_point.size(); ++o) {
    if (m.obs_point[o] != p) continue;
    m.obs_disabled[o] = have < want ? 0 : 1;
    ++have;
  }
  if (have < want) printf("FAIL point %d has only %d observations\n", p, have), ++g_fail;
}

static void CheckPlan(Map& m, const std::vector<int32_t>& points) {
  sg_map mv = m.view();
  PointsPlan plan;
  PlanPoints(mv, points.data(), (int32_t)points.size(), &plan);
  const int n = (int)points.size();
  CHECK((int)plan.off.size() == n + 1);
  CHECK((int)plan.points.size() == n);
  CHECK(plan.off[0] == 0);
  if (n == 0) {
    CHECK(plan.obs.empty() && plan.frames.empty() && plan.k.empty() && plan.num_run == 0);
    return;
  }
  int num_run = 0;
  for (int i = 0; i < n; ++i) {
    const int p = points[i];
    std::vector<int> keep;   // brute force: the enabled observations of p, in map order
    for (int o = 0; o < mv.num_obs; ++o)
      if (m.obs_point[o] == p && !m.obs_disabled[o]) keep.push_back(o);
    CHECK(plan.off[i + 1] - plan.off[i] == (int)keep.size());
    if (plan.off[i + 1] - plan.off[i] != (int)keep.size()) return;
    for (size_t j = 0; j < keep.size(); ++j) {
      const PointObs& r = plan.obs[plan.off[i] + j];
      const int o = keep[j];
      CHECK(r.u == m.obs_pt[2 * o] && r.v == m.obs_pt[2 * o + 1]);
      CHECK(r.frame == m.obs_frame[o]);
    }
    const PointStart& ps = plan.points[i];
    CHECK(std::memcmp(ps.X, &m.X[4 * p], 4 * sizeof(double)) == 0);
    CHECK(ps.run == ((int)keep.size() >= 2 ? 1 : 0));
    num_run += (int)keep.size() >= 2;
  }
  CHECK((int)plan.obs.size() == plan.off[n]);
  CHECK(plan.num_run == num_run);
  CHECK((int)plan.frames.size() == mv.num_frames);
  for (int f = 0; f < mv.num_frames && f < (int)plan.frames.size(); ++f) {
    const PointFrame& pf = plan.frames[f];
    CHECK(std::memcmp(pf.q, &m.q[4 * f], 4 * sizeof(double)) == 0);
    CHECK(std::memcmp(pf.t, &m.t[3 * f], 3 * sizeof(double)) == 0);
    CHECK(pf.camera == m.frame_camera[f]);
  }
  CHECK(plan.k == m.k);
}

template <typename Fn>
static bool Rejects(Fn fn) {
  try {
    fn();
  } catch (const Error& e) {
    return e.code == SG_EINVAL;
  }
  return false;
}

int main() {
  const int F = 12, P = 60;
  for (uint64_t seed = 1; seed <= 3; ++seed) {
    g_case = "seed " + std::to_string(seed);
    Map m = MakeMap(seed, F, P);
    ForceEnabled(m, kNone, 0);
    ForceEnabled(m, kOne, 1);
    ForceEnabled(m, kTwo, 2);
    std::vector<int32_t> all, rev;
    for (int p = 0; p < P; ++p) all.push_back(p);
    rev.assign(all.rbegin(), all.rend());
    CheckPlan(m, all);
    CheckPlan(m, rev);
    CheckPlan(m, {kEvery});
    CheckPlan(m, {kNone, kOne});   // nothing runs
    CheckPlan(m, {kTwo, kEvery, kOne, 0, 59});
    CheckPlan(m, {});
    {
      sg_map mv = m.view();
      PointsPlan plan;
      // a point observed by every frame, all enabled; and the upload is the observations used, not the map
      const int32_t every[1] = {kEvery};
      PlanPoints(mv, every, 1, &plan);
      CHECK((int)plan.obs.size() == F && plan.num_run == 1);
      for (int f = 0; f < F && f < (int)plan.obs.size(); ++f) CHECK(plan.obs[f].frame == f);
      const int32_t two[1] = {kTwo};
      PlanPoints(mv, two, 1, &plan);
      CHECK(plan.obs.size() == 2 && plan.points.size() == 1 && plan.num_run == 1);
      const int32_t one[2] = {kOne, kNone};
      PlanPoints(mv, one, 2, &plan);
      CHECK(plan.obs.size() == 1 && plan.num_run == 0 && plan.points[0].run == 0 && plan.points[1].run == 0);
    }
    // rejected lists: out of range, negative, duplicate, null, negative count
    sg_map mv = m.view();
    PointsPlan plan;
    const int32_t hi[2] = {1, P}, neg[1] = {-1}, dup[3] = {4, 5, 4};
    CHECK(Rejects([&] { PlanPoints(mv, hi, 2, &plan); }));
    CHECK(Rejects([&] { PlanPoints(mv, neg, 1, &plan); }));
    CHECK(Rejects([&] { PlanPoints(mv, dup, 3, &plan); }));
    CHECK(Rejects([&] { PlanPoints(mv, nullptr, 2, &plan); }));
    CHECK(Rejects([&] { PlanPoints(mv, hi, -1, &plan); }));
    // a map whose indices are out of range is rejected, not read
    const int32_t some[1] = {kEvery};
    {
      Map bad = m;
      bad.obs_point[5] = P;
      sg_map bv = bad.view();
      CHECK(Rejects([&] { PlanPoints(bv, some, 1, &plan); }));
    }
    {
      Map bad = m;
      bad.obs_frame[5] = F;
      sg_map bv = bad.view();
      CHECK(Rejects([&] { PlanPoints(bv, some, 1, &plan); }));
    }
    {
      Map bad = m;
      bad.obs_frame[3] = -1;
      sg_map bv = bad.view();
      CHECK(Rejects([&] { PlanPoints(bv, some, 1, &plan); }));
    }
    {
      Map bad = m;
      bad.frame_camera[F - 1] = 2;
      sg_map bv = bad.view();
      CHECK(Rejects([&] { PlanPoints(bv, some, 1, &plan); }));
    }
  }
  if (g_fail) {
    printf("points_plan_check: %d failures\n", g_fail);
    return 1;
  }
  printf("points_plan_check OK\n");
  return 0;
}
