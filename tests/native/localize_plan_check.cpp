// CPU check of what sg_slam_localize_frames adds to the pose planner (csrc/pose_plan.cpp): the run rule
// kLocalizeMinObs = 4 passed as min_obs, and each record's observation index (with_obs_index), recomputed by brute
// force on generated maps whose observations are not grouped by frame.  The defaults stay sg_slam_solve_frame_poses':
// run from kPoseMinObs = 3 records, no index list.  Built under AddressSanitizer and UBSan by
// tests/test_localize_plan.py.  No GPU, no HIP.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.h"
#include "pose_plan.h"

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
  // frame f gets exactly want[f] usable observations, plus disabled ones and ones of unusable points, interleaved
  Map(const std::vector<int>& want, uint64_t seed) {
    Lcg r{seed};
    const int F = (int)want.size(), P = 40;
    k.assign(14, 1.0);
    q.assign(4 * F, 0.5);
    t.assign(3 * F, 2.0);
    cam.assign(F, 0);
    prev.assign(F, -1);
    X.resize(4 * P);
    for (double& x : X) x = (double)(r.next() % 1000);
    unc.assign(P, 1.0);
    flags.assign(P, 0);
    for (int p = 0; p < P; p += 7) flags[p] = 1 << SG_NO_BASELINE;   // unusable points
    std::vector<int> left(want);
    for (bool any = true; any;) {
      any = false;
      for (int f = 0; f < F; ++f) {
        if (r.next() % 3 == 0) {   // a record that does not count
          int p = (int)(r.next() % P);
          const bool disabled = r.next() % 2;
          if (!disabled) p = p / 7 * 7;   // enabled, so its point must be unusable
          add(f, p, disabled, r);
        }
        if (left[f] > 0) {
          int p = (int)(r.next() % P);
          if (p % 7 == 0) p += 1;
          add(f, p, false, r);
          --left[f];
          any = true;
        }
      }
    }
    err.assign(pt.size(), 0.0);
    m.num_cameras = 2; m.k = k.data();
    m.num_frames = F; m.q = q.data(); m.t = t.data(); m.frame_camera = cam.data(); m.frame_prev = prev.data();
    m.num_points = P; m.X = X.data(); m.point_flags = flags.data(); m.point_uncertainty = unc.data();
    m.num_obs = (int32_t)of.size(); m.obs_pt = pt.data(); m.obs_frame = of.data(); m.obs_point = op.data();
    m.obs_disabled = dis.data(); m.obs_error = err.data();
  }
  void add(int f, int p, bool disabled, Lcg& r) {
    of.push_back(f);
    op.push_back(p);
    dis.push_back(disabled);
    pt.push_back((double)(r.next() % 640));
    pt.push_back((double)(r.next() % 480));
  }
};

}  // namespace

int main() {
  static_assert(sg::kLocalizeMinObs == 4 && sg::kPoseMinObs == 3, "run rules");
  const std::vector<int> want = {0, 1, 2, 3, 4, 5, 17, 3, 4};
  for (uint64_t seed = 1; seed <= 20; ++seed) {
    Map mp(want, seed);
    const std::vector<int32_t> frames = {8, 3, 4, 0, 6, 5, 2, 7, 1};
    const int n = (int)frames.size();
    sg::PosePlan loc, def;
    sg::PlanPoses(mp.m, frames.data(), n, false, &loc, sg::kLocalizeMinObs, true);
    sg::PlanPoses(mp.m, frames.data(), n, false, &def);
    CHECK(def.obs.empty(), "default plan carries an index list");
    CHECK(loc.off == def.off && loc.records.size() == def.records.size(), "record ranges differ");
    CHECK(loc.obs.size() == loc.records.size(), "index list size");
    int run_loc = 0, run_def = 0;
    for (int i = 0; i < n; ++i) {
      const int f = frames[i], cnt = loc.off[i + 1] - loc.off[i];
      CHECK(cnt == want[f], "frame %d: %d records, planted %d", f, cnt, want[f]);
      CHECK(loc.frames[i].run == (cnt >= 4), "frame %d: localize run %d at %d records", f, loc.frames[i].run, cnt);
      CHECK(def.frames[i].run == (cnt >= 3), "frame %d: default run %d at %d records", f, def.frames[i].run, cnt);
      run_loc += cnt >= 4;
      run_def += cnt >= 3;
      // brute force: the usable observations of f in map order
      int at = loc.off[i];
      for (int o = 0; o < mp.m.num_obs; ++o) {
        if (mp.of[o] != f || mp.dis[o] || (mp.flags[mp.op[o]] & (1 << SG_NO_BASELINE))) continue;
        const bool in_range = at < loc.off[i + 1];
        CHECK(in_range, "frame %d: more usable observations than records", f);
        if (!in_range) break;
        CHECK(loc.obs[at] == o, "frame %d record %d: observation %d, expected %d", f, at - loc.off[i], loc.obs[at], o);
        const sg::PoseRecord& rc = loc.records[at];
        CHECK(rc.u == mp.pt[2 * o] && rc.v == mp.pt[2 * o + 1] &&
                  std::memcmp(rc.X, &mp.X[4 * mp.op[o]], sizeof(rc.X)) == 0 &&
                  std::memcmp(&rc, &def.records[at], sizeof(rc)) == 0,
              "frame %d record %d: contents", f, at - loc.off[i]);
        ++at;
      }
      CHECK(at == loc.off[i + 1], "frame %d: %d records matched of %d", f, at - loc.off[i], cnt);
    }
    CHECK(loc.num_run == run_loc && def.num_run == run_def, "num_run %d / %d", loc.num_run, def.num_run);
  }
  if (g_fail) {
    std::printf("localize_plan_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("localize_plan_check OK\n");
  return 0;
}
