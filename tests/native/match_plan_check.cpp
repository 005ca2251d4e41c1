// CPU check of csrc/match_plan.cpp, the host-only planner of sg_slam_match_by_projection: on generated maps, the frame
// records, the gathered points, the skip_observed exclusion mask (frames listed twice, disabled observations, unlisted
// points), the work list and the launch shapes against brute force; ResolveMatches against a brute-force restatement
// of the acceptance and uniqueness rule; K == 0, np == 0 and n == 0; and every SG_EINVAL case of the contract.  Prints
// the constants that tests/match_cases.py restates.  Built under AddressSanitizer and UBSan by
// tests/test_match_plan.py.  No GPU, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "match_plan.h"

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
  double unit() { return (double)(next() % 2000001) / 1e6 - 1.0; }
};

const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kInf = std::numeric_limits<double>::infinity();

struct Map {
  std::vector<double> k, q, t, X;
  std::vector<int32_t> cam, of, op, od;
  sg_map m{};
  Map(int C, int F, int P, int M, uint64_t seed) {
    Lcg r{seed};
    k.resize(7 * (size_t)C);
    q.resize(4 * (size_t)F);
    t.resize(3 * (size_t)F);
    X.resize(4 * (size_t)P);
    for (double& v : k) v = r.unit();
    for (double& v : q) v = r.unit();
    for (double& v : t) v = 1000.0 * r.unit();
    for (double& v : X) v = 3000.0 * r.unit();
    if (P > 2) X[4 * 2 + 1] = kNaN;   // the planner copies locations as they are
    cam.resize(F);
    for (int f = 0; f < F; ++f) cam[f] = (int)(r.next() % C);
    of.resize(M);
    op.resize(M);
    od.resize(M);
    for (int o = 0; o < M; ++o) {
      of[o] = (int)(r.next() % F);
      op[o] = (int)(r.next() % P);
      od[o] = r.next() % 3 == 0 ? (int)(1 + r.next() % 2) : 0;   // disabled: any non-zero value
    }
    m.num_cameras = C;
    m.k = k.data();
    m.num_frames = F;
    m.q = q.data();
    m.t = t.data();
    m.frame_camera = cam.data();
    m.num_points = P;
    m.X = X.data();
    m.num_obs = M;
    m.obs_frame = of.data();
    m.obs_point = op.data();
    m.obs_disabled = od.data();
  }
};

sg_match_options defaults() {
  sg_match_options o{};
  o.radius_px = 12.0;
  o.max_dist = 64;
  o.ratio_percent = 80;
  o.skip_observed = 1;
  return o;
}

struct Call {
  std::vector<int32_t> frames, off, points;
  std::vector<double> xy;
  std::vector<uint64_t> kd, pd;
};

int plan_code(const sg_map* m, const int32_t* frames, int n, const int32_t* off, const double* xy, const uint64_t* kd,
              const int32_t* points, int np, const uint64_t* pd, const sg_match_options* o,
              sg::MatchPlan* keep = nullptr) {
  sg::MatchPlan plan;
  try {
    sg::PlanMatch(m, frames, n, off, xy, kd, points, np, pd, o, &plan);
  } catch (const sg::Error& e) {
    return e.code;
  }
  if (keep) *keep = plan;
  return SG_OK;
}

int plan_code(const sg_map* m, const Call& c, const sg_match_options* o, sg::MatchPlan* keep = nullptr) {
  return plan_code(m, c.frames.data(), (int)c.frames.size(), c.off.data(), c.xy.data(), c.kd.data(), c.points.data(),
                   (int)c.points.size(), c.pd.data(), o, keep);
}

// n listed frames (with repeats), keypoint counts that include 0, 1, kMatchChunk and kMatchChunk + 1, np points in a
// shuffled order.
Call make_call(const Map& map, int n, int np, uint64_t seed) {
  Lcg r{seed};
  Call c;
  c.off.push_back(0);
  const int special[5] = {0, 1, sg::kMatchChunk, sg::kMatchChunk + 1, 3 * sg::kMatchChunk - 1};
  for (int i = 0; i < n; ++i) {
    c.frames.push_back(i == 1 && n > 1 ? c.frames[0] : (int)(r.next() % map.m.num_frames));   // a frame listed twice
    const int k = i < 5 ? special[i] : (int)(r.next() % 700);
    c.off.push_back(c.off.back() + k);
  }
  c.xy.assign(2 * (size_t)c.off.back() + 2, 1.0);
  c.kd.assign(4 * (size_t)c.off.back() + 4, 7u);
  std::vector<int32_t> all(map.m.num_points);
  for (int p = 0; p < map.m.num_points; ++p) all[p] = p;
  for (int p = map.m.num_points - 1; p > 0; --p) std::swap(all[p], all[r.next() % (p + 1)]);
  c.points.assign(all.begin(), all.begin() + np);
  c.pd.assign(4 * (size_t)np + 4, 9u);
  return c;
}

void check_plan(int C, int F, int P, int M, int n, int np, int skip, uint64_t seed) {
  Map map(C, F, P, M, seed);
  const Call c = make_call(map, n, np, seed * 31 + 5);
  sg_match_options o = defaults();
  o.skip_observed = skip;
  sg::MatchPlan plan;
  const int code = plan_code(&map.m, c, &o, &plan);
  CHECK(code == SG_OK, "plan failed with %d", code);
  if (code != SG_OK) return;
  const int K = c.off.back();
  CHECK(plan.n == n && plan.np == np && plan.K == K, "sizes");
  CHECK(plan.launch == (K > 0 && np > 0), "launch");
  CHECK(plan.words == (np + 31) / 32 && plan.slices == (np + sg::kMatchSlice - 1) / sg::kMatchSlice &&
            plan.project_blocks == (np + 255) / 256,
        "launch shapes");
  CHECK((int)plan.frames.size() == n && plan.X.size() == 4 * (size_t)np && plan.excl.size() == (size_t)n * plan.words,
        "array sizes");
  for (int i = 0; i < n; ++i) {
    const int f = c.frames[i];
    const sg::MatchFrame& mf = plan.frames[i];
    CHECK(std::memcmp(mf.q, &map.q[4 * f], 32) == 0 && std::memcmp(mf.t, &map.t[3 * f], 24) == 0 &&
              std::memcmp(mf.k, &map.k[7 * map.cam[f]], 56) == 0,
          "frame record %d", i);
  }
  for (int j = 0; j < np; ++j)
    CHECK(std::memcmp(&plan.X[4 * (size_t)j], &map.X[4 * (size_t)c.points[j]], 32) == 0, "point %d", j);
  // the exclusion mask by brute force, bit by bit; bits beyond np are clear
  long set = 0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 32 * plan.words; ++j) {
      bool want = false;
      if (skip && j < np)
        for (int ob = 0; ob < M; ++ob)
          want = want || (map.of[ob] == c.frames[i] && map.op[ob] == c.points[j] && map.od[ob] == 0);
      const bool got = (plan.excl[(size_t)i * plan.words + (j >> 5)] >> (j & 31)) & 1u;
      CHECK(want == got, "exclusion bit of slot %d position %d: want %d", i, j, (int)want);
      set += got;
    }
  if (skip && M >= 300 * F && np == P) CHECK(set > 0, "the generated map excludes nothing");
  // the work list: every keypoint once, frames in listed order, chunks in keypoint order, none empty
  std::vector<int> seen((size_t)K, 0);
  int32_t last_slot = -1, last_kp = -1;
  for (const sg::MatchChunk& ch : plan.chunks) {
    CHECK(ch.slot >= last_slot && ch.kp0 > last_kp && ch.count >= 1 && ch.count <= sg::kMatchChunk, "chunk order");
    CHECK(ch.slot >= 0 && ch.slot < n && ch.kp0 >= c.off[ch.slot] && ch.kp0 + ch.count <= c.off[ch.slot + 1],
          "chunk outside its frame");
    CHECK(ch.kp0 + ch.count == c.off[ch.slot + 1] || ch.count == sg::kMatchChunk, "a short chunk that is not the last");
    for (int k = ch.kp0; k < ch.kp0 + ch.count && k < K; ++k) ++seen[k];
    last_slot = ch.slot;
    last_kp = ch.kp0;
  }
  for (int k = 0; k < K; ++k) CHECK(seen[k] == 1, "keypoint %d in %d chunks", k, seen[k]);
}

void check_resolve(uint64_t seed, int max_dist, int ratio) {
  Lcg r{seed};
  const int n = 6;
  std::vector<int32_t> off(1, 0);
  for (int i = 0; i < n; ++i) off.push_back(off.back() + (i == 2 ? 0 : (int)(r.next() % 400)));
  const int K = off.back();
  std::vector<int32_t> bp(K), bd(K), sd(K), nc(K);
  for (int k = 0; k < K; ++k) {
    nc[k] = (int)(r.next() % 4);
    bp[k] = nc[k] ? (int)(r.next() % 40) : -1;   // few points: many claimants each
    bd[k] = nc[k] ? (int)(r.next() % 90) : -1;
    sd[k] = nc[k] > 1 ? bd[k] + (int)(r.next() % 30) : -1;
  }
  sg_match_options o = defaults();
  o.max_dist = max_dist;
  o.ratio_percent = ratio;
  std::vector<int32_t> match((size_t)K + 1, 7);
  std::vector<sg_match_result> res(n);
  for (sg_match_result& x : res) x.num_keypoints = x.num_projected = 77;
  sg::ResolveMatches(off.data(), n, bp.data(), bd.data(), sd.data(), nc.data(), o, match.data(), res.data());
  CHECK(match[K] == 7, "wrote past the keypoints");
  for (int i = 0; i < n; ++i) {
    int with = 0, matched = 0;
    for (int k = off[i]; k < off[i + 1]; ++k) {
      with += nc[k] > 0;
      auto accepted = [&](int a) {
        return bp[a] >= 0 && bd[a] <= max_dist && (sd[a] < 0 || 100 * bd[a] <= ratio * sd[a]);
      };
      int want = -1;
      if (accepted(k)) {
        want = bp[k];
        for (int a = off[i]; a < off[i + 1]; ++a)   // a better claimant of the same point, in this frame only
          if (a != k && accepted(a) && bp[a] == bp[k] && (bd[a] < bd[k] || (bd[a] == bd[k] && a < k))) want = -1;
      }
      CHECK(match[k] == want, "match of keypoint %d: %d, want %d", k, match[k], want);
      matched += want >= 0;
    }
    CHECK(res[i].num_with_candidates == with && res[i].num_matched == matched, "counts of frame %d", i);
    CHECK(res[i].num_keypoints == 77 && res[i].num_projected == 77, "fields that are not ResolveMatches'");
  }
  // results may be null
  sg::ResolveMatches(off.data(), n, bp.data(), bd.data(), sd.data(), nc.data(), o, match.data(), nullptr);
}

void check_errors() {
  Map map(2, 6, 50, 200, 11);
  const Call c = make_call(map, 4, 30, 3);
  const sg_match_options o = defaults();
  const int n = 4, np = 30;
  const int32_t *fr = c.frames.data(), *off = c.off.data(), *pts = c.points.data();
  const double* xy = c.xy.data();
  const uint64_t *kd = c.kd.data(), *pd = c.pd.data();
  CHECK(plan_code(&map.m, c, &o) == SG_OK, "the base call");
  CHECK(plan_code(nullptr, fr, n, off, xy, kd, pts, np, pd, &o) == SG_EINVAL, "null map");
  CHECK(plan_code(&map.m, fr, n, off, xy, kd, pts, np, pd, nullptr) == SG_EINVAL, "null options");
  CHECK(plan_code(&map.m, fr, -1, off, xy, kd, pts, np, pd, &o) == SG_EINVAL, "n < 0");
  CHECK(plan_code(&map.m, fr, n, off, xy, kd, pts, -1, pd, &o) == SG_EINVAL, "np < 0");
  CHECK(plan_code(&map.m, nullptr, n, off, xy, kd, pts, np, pd, &o) == SG_EINVAL, "null frames");
  CHECK(plan_code(&map.m, fr, n, nullptr, xy, kd, pts, np, pd, &o) == SG_EINVAL, "null kp_offset");
  CHECK(plan_code(&map.m, fr, n, off, nullptr, kd, pts, np, pd, &o) == SG_EINVAL, "null kp_xy");
  CHECK(plan_code(&map.m, fr, n, off, xy, nullptr, pts, np, pd, &o) == SG_EINVAL, "null kp_desc");
  CHECK(plan_code(&map.m, fr, n, off, xy, kd, nullptr, np, pd, &o) == SG_EINVAL, "null points");
  CHECK(plan_code(&map.m, fr, n, off, xy, kd, pts, np, nullptr, &o) == SG_EINVAL, "null point_desc");
  // lists that would not be read may be null: K == 0, np == 0, n == 0
  const int32_t zero_off[5] = {0, 0, 0, 0, 0};
  sg::MatchPlan plan;
  CHECK(plan_code(&map.m, fr, n, zero_off, nullptr, nullptr, pts, np, pd, &o, &plan) == SG_OK && !plan.launch &&
            plan.chunks.empty() && plan.K == 0,
        "K == 0");
  CHECK(plan_code(&map.m, fr, n, off, xy, kd, nullptr, 0, nullptr, &o, &plan) == SG_OK && !plan.launch &&
            plan.slices == 0 && plan.words == 0 && plan.excl.empty() && !plan.chunks.empty(),
        "np == 0");
  CHECK(plan_code(&map.m, nullptr, 0, nullptr, nullptr, nullptr, nullptr, np, nullptr, &o, &plan) == SG_OK &&
            !plan.launch && plan.frames.empty(),
        "n == 0");
  {
    std::vector<int32_t> b(c.off);
    b[0] = 1;
    CHECK(plan_code(&map.m, fr, n, b.data(), xy, kd, pts, np, pd, &o) == SG_EINVAL, "kp_offset[0] != 0");
    b = c.off;
    b[2] = b[1] - 1;
    CHECK(plan_code(&map.m, fr, n, b.data(), xy, kd, pts, np, pd, &o) == SG_EINVAL, "decreasing kp_offset");
    const int32_t big[2] = {0, sg::kMatchMaxKeypoints + 1};
    CHECK(plan_code(&map.m, fr, 1, big, xy, kd, pts, np, pd, &o) == SG_EINVAL, "K > 2^20");   // (found before xy is read)
  }
  for (int32_t bad : {-1, 6, 0x7fffffff}) {
    std::vector<int32_t> b(c.frames);
    b[2] = bad;
    CHECK(plan_code(&map.m, b.data(), n, off, xy, kd, pts, np, pd, &o) == SG_EINVAL, "frame %d", bad);
  }
  for (int32_t bad : {-1, 50, 0x7fffffff}) {
    std::vector<int32_t> b(c.points);
    b[7] = bad;
    CHECK(plan_code(&map.m, fr, n, off, xy, kd, b.data(), np, pd, &o) == SG_EINVAL, "point %d", bad);
  }
  {
    std::vector<int32_t> b(c.points);
    b[9] = b[3];
    CHECK(plan_code(&map.m, fr, n, off, xy, kd, b.data(), np, pd, &o) == SG_EINVAL, "a point listed twice");
  }
  auto with = [&](auto set) {
    sg_match_options b = defaults();
    set(b);
    // option errors are found with n == 0 too
    return plan_code(&map.m, fr, n, off, xy, kd, pts, np, pd, &b) == SG_EINVAL &&
           plan_code(&map.m, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &b) == SG_EINVAL;
  };
  for (double bad : {0.0, -1.0, kNaN, kInf, -kInf})
    CHECK(with([&](sg_match_options& b) { b.radius_px = bad; }), "radius_px %g", bad);
  CHECK(with([](sg_match_options& b) { b.width = -1; b.height = 480; }), "negative width");
  CHECK(with([](sg_match_options& b) { b.width = 640; b.height = -1; }), "negative height");
  CHECK(with([](sg_match_options& b) { b.width = -640; b.height = -480; }), "both negative");
  CHECK(with([](sg_match_options& b) { b.width = 640; }), "only the height zero");
  CHECK(with([](sg_match_options& b) { b.height = 480; }), "only the width zero");
  for (int bad : {-1, 257}) CHECK(with([&](sg_match_options& b) { b.max_dist = bad; }), "max_dist %d", bad);
  for (int bad : {0, -5, 101}) CHECK(with([&](sg_match_options& b) { b.ratio_percent = bad; }), "ratio_percent %d", bad);
  for (int ok : {0, 256}) {
    sg_match_options b = defaults();
    b.max_dist = ok;
    b.ratio_percent = ok ? 100 : 1;
    b.width = 640;
    b.height = 480;
    CHECK(plan_code(&map.m, c, &b) == SG_OK, "the ends of the ranges are valid");
  }
  {   // n * np > 2^22: a large map and a frame listed often; exactly 2^22 passes
    Map big(1, 2, 1 << 12, 0, 5);
    std::vector<int32_t> p(1 << 12), f((1 << 10) + 1, 1), z((1 << 10) + 2, 0);
    for (int j = 0; j < (1 << 12); ++j) p[j] = j;
    std::vector<uint64_t> d(4 << 12, 1u);
    CHECK(plan_code(&big.m, f.data(), 1 << 10, z.data(), nullptr, nullptr, p.data(), 1 << 12, d.data(), &o) == SG_OK,
          "n np == 2^22");
    CHECK(plan_code(&big.m, f.data(), (1 << 10) + 1, z.data(), nullptr, nullptr, p.data(), 1 << 12, d.data(), &o) ==
              SG_EINVAL,
          "n np > 2^22");
  }
  // maps that cannot be read
  auto broken = [&](auto set, const sg_match_options& opt) {
    Map b(2, 6, 50, 200, 11);
    set(b);
    return plan_code(&b.m, c, &opt);
  };
  CHECK(broken([](Map& b) { b.m.q = nullptr; }, o) == SG_EINVAL, "null q");
  CHECK(broken([](Map& b) { b.m.t = nullptr; }, o) == SG_EINVAL, "null t");
  CHECK(broken([](Map& b) { b.m.k = nullptr; }, o) == SG_EINVAL, "null k");
  CHECK(broken([](Map& b) { b.m.frame_camera = nullptr; }, o) == SG_EINVAL, "null frame_camera");
  CHECK(broken([](Map& b) { b.m.X = nullptr; }, o) == SG_EINVAL, "null X");
  CHECK(broken([&](Map& b) { b.cam[c.frames[3]] = 2; }, o) == SG_EINVAL, "camera out of range");
  CHECK(broken([&](Map& b) { b.cam[c.frames[3]] = -1; }, o) == SG_EINVAL, "negative camera");
  CHECK(broken([](Map& b) { b.m.num_obs = -1; }, o) == SG_EINVAL, "negative num_obs");
  sg_match_options noskip = defaults();
  noskip.skip_observed = 0;
  CHECK(broken([](Map& b) { b.m.obs_frame = nullptr; }, o) == SG_EINVAL, "null obs_frame");
  CHECK(broken([](Map& b) { b.m.obs_point = nullptr; }, o) == SG_EINVAL, "null obs_point");
  CHECK(broken([](Map& b) { b.m.obs_disabled = nullptr; }, o) == SG_EINVAL, "null obs_disabled");
  CHECK(broken([](Map& b) { b.of[17] = 6; }, o) == SG_EINVAL, "obs_frame out of range");
  CHECK(broken([](Map& b) { b.op[17] = -1; }, o) == SG_EINVAL, "obs_point out of range");
  // ... which are not read without skip_observed
  CHECK(broken([](Map& b) { b.m.obs_frame = b.m.obs_point = nullptr; b.m.obs_disabled = nullptr; }, noskip) == SG_OK,
        "observations are not read without skip_observed");
  CHECK(broken([](Map& b) { b.of[17] = 6; }, noskip) == SG_OK, "observation indices are not read without skip_observed");
  // the planner needs neither flags nor pixels nor frame_prev (null in Map)
}

}  // namespace

int main() {
  std::printf("kMatchChunk %d kMatchTile %d kMatchSlice %d kMatchKeyShift %d\n", sg::kMatchChunk, sg::kMatchTile,
              sg::kMatchSlice, sg::kMatchKeyShift);
  check_plan(2, 10, 500, 3000, 8, 500, 1, 1);
  check_plan(2, 10, 500, 3000, 8, 333, 1, 2);     // some points unlisted, np no multiple of 32
  check_plan(3, 7, 2100, 4000, 5, 2100, 1, 3);    // more than two slices
  check_plan(2, 10, 500, 3000, 8, 500, 0, 4);     // no exclusion
  check_plan(1, 4, 64, 0, 3, 64, 1, 5);           // a map without observations
  check_plan(2, 10, 500, 3000, 1, 1, 1, 6);
  for (uint64_t s = 1; s <= 4; ++s) check_resolve(s, 64, 80);
  check_resolve(9, 0, 100);
  check_resolve(10, 256, 1);
  check_errors();
  if (g_fail) {
    std::printf("match_plan_check FAILED: %d checks\n", g_fail);
    return 1;
  }
  std::printf("match_plan_check OK\n");
  return 0;
}
