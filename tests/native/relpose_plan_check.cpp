// CPU check of csrc/relpose_plan.cpp, the host-only planner of sg_slam_relative_poses: the record lists of generated
// maps (disabled observations, a point seen twice in one frame, observations not grouped by frame) against a brute
// force restatement; a pair with 7 records; n = 0; the launch shape; and every SG_EINVAL case of the contract.  Built
// under AddressSanitizer and UBSan by tests/test_relpose_plan.py.  No GPU, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "common.h"
#include "relpose_plan.h"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      if (++g_fail <= 20) {                              \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                        \
        std::printf("\n");                               \
      }                                                  \
    }                                                    \
  } while (0)

struct Lcg {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
};

struct Map {
  std::vector<double> k, q, t, X, unc, pt, err;
  std::vector<int32_t> cam, prev, flags, of, op, dis;
  sg_map m{};
  Map(int F, int P, int M, uint64_t seed) {
    Lcg r{seed};
    k.assign(14, 1.0);
    for (int i = 0; i < 14; ++i) k[i] = 1.0 + i;
    q.assign(4 * F, 0.5);
    t.assign(3 * F, 2.0);
    cam.resize(F);
    for (int f = 0; f < F; ++f) cam[f] = f % 2;
    prev.assign(F, -1);
    X.assign(4 * P, 0.5);
    unc.assign(P, 1.0);
    flags.assign(P, 6);   // NO_BASELINE | NO_OBSERVATIONS: flags are not consulted
    for (int o = 0; o < M; ++o) {
      of.push_back((int32_t)(r.next() % F));
      op.push_back((int32_t)(r.next() % P));   // (a point is often seen twice in one frame)
      dis.push_back(r.next() % 4 == 0);
      pt.push_back((double)(r.next() % 640));
      pt.push_back((double)(r.next() % 480));
    }
    err.assign(pt.size(), 0.0);
    m.num_cameras = 2; m.k = k.data();
    m.num_frames = F; m.q = q.data(); m.t = t.data(); m.frame_camera = cam.data(); m.frame_prev = prev.data();
    m.num_points = P; m.X = X.data(); m.point_flags = flags.data(); m.point_uncertainty = unc.data();
    m.num_obs = (int32_t)of.size(); m.obs_pt = pt.data(); m.obs_frame = of.data(); m.obs_point = op.data();
    m.obs_disabled = dis.data(); m.obs_error = err.data();
  }
  int first(int f, int p) const {   // the first enabled observation of point p in frame f, or -1
    for (int o = 0; o < m.num_obs; ++o)
      if (of[o] == f && op[o] == p && !dis[o]) return o;
    return -1;
  }
};

int plan_code(const sg_map* m, const int32_t* pairs, int n, const sg_relpose_options* o) {
  sg::RelPlan plan;
  try {
    sg::PlanRelPoses(m, pairs, n, o, &plan);
  } catch (const sg::Error& e) {
    return e.code;
  }
  return SG_OK;
}

sg_relpose_options options() {
  sg_relpose_options o{};
  o.threshold_px = 2.0;
  o.max_hypotheses = 1024;
  o.min_inliers = 16;
  o.refine = 1;
  return o;
}

}  // namespace

int main() {
  const sg_relpose_options o = options();
  for (uint64_t seed = 1; seed <= 20; ++seed) {
    Map mp(6, 30, 400, seed);
    const std::vector<int32_t> pairs = {0, 1, 1, 2, 5, 3, 2, 0, 3, 4};
    const int n = 5;
    sg::RelPlan plan;
    sg::PlanRelPoses(&mp.m, pairs.data(), n, &o, &plan);
    CHECK(plan.H == 1024 && plan.S == 4 && plan.grid == 20, "launch shape %d %d %ld", plan.H, plan.S, (long)plan.grid);
    int run = 0;
    for (int i = 0; i < n; ++i) {
      const int a = pairs[2 * i], b = pairs[2 * i + 1];
      int at = plan.off[i];
      std::vector<char> seen(30, 0);
      for (int oa = 0; oa < mp.m.num_obs; ++oa) {
        if (mp.of[oa] != a || mp.dis[oa] || seen[mp.op[oa]]) continue;
        seen[mp.op[oa]] = 1;
        const int ob = mp.first(b, mp.op[oa]);
        if (ob < 0) continue;
        const bool in_range = at < plan.off[i + 1];
        CHECK(in_range, "pair %d: more records than planned", i);
        if (!in_range) break;
        CHECK(plan.obs[2 * at] == oa && plan.obs[2 * at + 1] == ob, "pair %d record %d: observations %d %d, expected %d %d",
              i, at - plan.off[i], plan.obs[2 * at], plan.obs[2 * at + 1], oa, ob);
        CHECK(plan.records[4 * at] == mp.pt[2 * oa] && plan.records[4 * at + 1] == mp.pt[2 * oa + 1] &&
                  plan.records[4 * at + 2] == mp.pt[2 * ob] && plan.records[4 * at + 3] == mp.pt[2 * ob + 1],
              "pair %d record %d: pixels", i, at - plan.off[i]);
        ++at;
      }
      CHECK(at == plan.off[i + 1], "pair %d: %d records matched of %d", i, at - plan.off[i], plan.off[i + 1] - plan.off[i]);
      const sg::RelPair& rp = plan.pairs[i];
      CHECK(rp.a == a && rp.b == b && rp.run == (plan.off[i + 1] - plan.off[i] >= 8), "pair %d: header", i);
      CHECK(rp.ka[3] == mp.k[7 * mp.cam[a] + 3] && rp.kb[6] == mp.k[7 * mp.cam[b] + 6], "pair %d: intrinsics", i);
      run += rp.run;
    }
    CHECK(plan.num_run == run, "num_run %d, expected %d", plan.num_run, run);
    CHECK(plan.records.size() == 4 * (size_t)plan.off[n] && plan.obs.size() == 2 * (size_t)plan.off[n], "array sizes");
  }
  {   // exactly 7 and exactly 8 records
    for (int cnt = 7; cnt <= 8; ++cnt) {
      Map mp(2, 10, 0, 1);
      for (int f = 0; f < 2; ++f)
        for (int p = 0; p < cnt; ++p) {
          mp.of.push_back(f); mp.op.push_back(p); mp.dis.push_back(0);
          mp.pt.push_back(p); mp.pt.push_back(f);
        }
      mp.m.num_obs = (int32_t)mp.of.size();
      mp.m.obs_pt = mp.pt.data(); mp.m.obs_frame = mp.of.data(); mp.m.obs_point = mp.op.data();
      mp.m.obs_disabled = mp.dis.data();
      const int32_t pr[2] = {0, 1};
      sg::RelPlan plan;
      sg::PlanRelPoses(&mp.m, pr, 1, &o, &plan);
      CHECK(plan.off[1] == cnt && plan.pairs[0].run == (cnt >= 8) && plan.num_run == (cnt >= 8), "%d records: run %d",
            cnt, plan.pairs[0].run);
    }
  }
  Map mp(4, 10, 50, 3);
  const int32_t ok[2] = {0, 1};
  sg::RelPlan empty;
  sg::PlanRelPoses(&mp.m, nullptr, 0, &o, &empty);
  CHECK(empty.off.size() == 1 && empty.off[0] == 0 && empty.pairs.empty() && empty.grid == 0, "n = 0");
  CHECK(plan_code(&mp.m, ok, 1, &o) == SG_OK, "a good call");
  CHECK(plan_code(nullptr, ok, 1, &o) == SG_EINVAL, "null map");
  CHECK(plan_code(&mp.m, ok, 1, nullptr) == SG_EINVAL, "null options");
  CHECK(plan_code(&mp.m, nullptr, 1, &o) == SG_EINVAL, "null pairs");
  CHECK(plan_code(&mp.m, ok, -1, &o) == SG_EINVAL, "n < 0");
  for (double bad : {0.0, -1.0, std::nan("")}) {
    sg_relpose_options b = o;
    b.threshold_px = bad;
    CHECK(plan_code(&mp.m, ok, 1, &b) == SG_EINVAL && plan_code(&mp.m, nullptr, 0, &b) == SG_EINVAL, "threshold %g", bad);
  }
  for (int bad : {0, -256}) {
    sg_relpose_options b = o;
    b.max_hypotheses = bad;
    CHECK(plan_code(&mp.m, ok, 1, &b) == SG_EINVAL, "max_hypotheses %d", bad);
  }
  for (double bad : {-1.0, std::nan("")}) {
    sg_relpose_options b = o;
    b.baseline = bad;
    CHECK(plan_code(&mp.m, ok, 1, &b) == SG_EINVAL, "baseline %g", bad);
  }
  const int32_t range1[2] = {0, 4}, range2[2] = {-1, 1}, same[2] = {2, 2}, twice[4] = {0, 1, 2, 1};
  CHECK(plan_code(&mp.m, range1, 1, &o) == SG_EINVAL && plan_code(&mp.m, range2, 1, &o) == SG_EINVAL, "frame range");
  CHECK(plan_code(&mp.m, same, 1, &o) == SG_EINVAL, "a == b");
  CHECK(plan_code(&mp.m, twice, 2, &o) == SG_EINVAL, "the same b twice");
  mp.cam[1] = 2;
  CHECK(plan_code(&mp.m, ok, 1, &o) == SG_EINVAL, "camera out of range");
  mp.cam[1] = 1;
  mp.m.k = nullptr;
  CHECK(plan_code(&mp.m, ok, 1, &o) == SG_EINVAL, "no intrinsics");
  {   // the hypothesis count: rounded up to 256, capped at 2^20
    Map m2(4, 10, 50, 3);
    sg_relpose_options b = o;
    sg::RelPlan plan;
    b.max_hypotheses = 1;
    sg::PlanRelPoses(&m2.m, ok, 1, &b, &plan);
    CHECK(plan.H == 256 && plan.S == 1, "H %d", plan.H);
    b.max_hypotheses = 257;
    sg::PlanRelPoses(&m2.m, ok, 1, &b, &plan);
    CHECK(plan.H == 512 && plan.S == 2, "H %d", plan.H);
    b.max_hypotheses = 0x7fffffff;
    sg::PlanRelPoses(&m2.m, ok, 1, &b, &plan);
    CHECK(plan.H == (1 << 20) && plan.S == 4096, "H %d", plan.H);
  }
  if (g_fail) {
    std::printf("relpose_plan_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("relpose_plan_check OK\n");
  return 0;
}
