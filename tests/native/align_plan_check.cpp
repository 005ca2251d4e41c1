// CPU check of csrc/align_plan.cpp, the host-only planner of sg_slam_align_points: the records of generated maps
// (unusable flags, non-finite coordinates, points at infinity, W of either sign and any 4-norm) against a brute-force
// restatement; the offsets, the sampler key and the N < 4 rule; empty groups; n = 0; the launch shape; and every
// SG_EINVAL case of the contract.  Built under AddressSanitizer and UBSan by tests/test_align_plan.py.  No GPU, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "align_plan.h"
#include "common.h"

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

// Points only: the planner must not read frames, observations or pixels (their pointers stay null).
struct Map {
  std::vector<double> X;
  std::vector<int32_t> flags;
  sg_map m{};
  Map(int P, uint64_t seed) {
    Lcg r{seed};
    X.resize(4 * (size_t)P);
    flags.assign(P, 0);
    for (int p = 0; p < P; ++p) {
      const double scale = (p % 3 == 0) ? 1.0 : (p % 3 == 1 ? 1e-3 : 250.0);   // any 4-norm
      for (int c = 0; c < 3; ++c) X[4 * p + c] = 3000.0 * r.unit() * scale;
      X[4 * p + 3] = (p % 5 == 0 ? -1.0 : 1.0) * scale;                         // W of either sign
      const uint32_t kind = r.next() % 16;
      if (kind == 0) flags[p] = 1 << SG_BAD_LOCATION;
      if (kind == 1) flags[p] = 1 << SG_NO_BASELINE;
      if (kind == 2) flags[p] = 1 << SG_NO_OBSERVATIONS;
      if (kind == 3) flags[p] = 1 << SG_BAD_FEATURE;
      if (kind == 4) flags[p] = 1 << SG_MISMATCHED;   // (usable)
      if (kind == 5) X[4 * p + r.next() % 4] = kNaN;
      if (kind == 6) X[4 * p + r.next() % 4] = r.next() % 2 ? kInf : -kInf;
      if (kind == 7) X[4 * p + 3] = 0.0;
      if (kind == 8) X[4 * p + 3] *= 1e-13;           // at infinity: |W| < 1e-9 |X|
    }
    m.num_points = P;
    m.X = X.data();
    m.point_flags = flags.data();
  }
  bool usable(int p, double* E) const {
    if (flags[p] & 0x17) return false;
    const double* x = &X[4 * (size_t)p];
    for (int c = 0; c < 4; ++c)
      if (!std::isfinite(x[c])) return false;
    const long double n2 = (long double)x[0] * x[0] + (long double)x[1] * x[1] + (long double)x[2] * x[2] +
                           (long double)x[3] * x[3];
    if (!(std::fabs((long double)x[3]) >= 1e-9L * std::sqrt(n2))) return false;
    for (int c = 0; c < 3; ++c) E[c] = x[c] / x[3];
    return true;
  }
};

sg_align_options defaults() {
  sg_align_options o{};
  o.threshold = 10.0;
  o.max_hypotheses = 1024;
  o.min_inliers = 8;
  o.refine = 1;
  o.min_gap = 1e-6;
  return o;
}

int plan_code(const sg_map* m, const int32_t* corr, const int32_t* off, int n, const sg_align_options* o) {
  sg::AlignPlan plan;
  try {
    sg::PlanAlign(m, corr, off, n, o, &plan);
  } catch (const sg::Error& e) {
    return e.code;
  }
  return SG_OK;
}

void check_records(int P, int n, uint64_t seed) {
  Map map(P, seed);
  Lcg r{seed * 77 + 1};
  std::vector<int32_t> corr, off(1, 0);
  for (int g = 0; g < n; ++g) {
    const int k = g == 1 ? 0 : (g == 2 ? 3 : (int)(r.next() % 90));   // an empty group, a group of three
    for (int j = 0; j < k; ++j) {
      const int a = (int)(r.next() % P);
      int b = (int)(r.next() % P);
      if (b == a) b = (a + 1) % P;
      corr.push_back(a);
      corr.push_back(b);
    }
    off.push_back((int32_t)(corr.size() / 2));
  }
  sg_align_options o = defaults();
  sg::AlignPlan plan;
  sg::PlanAlign(&map.m, corr.data(), off.data(), n, &o, &plan);
  CHECK((int)plan.off.size() == n + 1 && (int)plan.groups.size() == n && plan.off[0] == 0, "sizes");
  int run = 0, few = 0;
  size_t rpos = 0;
  for (int g = 0; g < n; ++g) {
    int cnt = 0;
    for (int j = off[g]; j < off[g + 1]; ++j) {
      double E[6];
      if (!map.usable(corr[2 * j], E) || !map.usable(corr[2 * j + 1], E + 3)) continue;
      const bool have = rpos < plan.rec_corr.size();
      CHECK(have && plan.rec_corr[rpos] == j, "group %d: record %zu is not correspondence %d", g, rpos, j);
      if (have)
        for (int c = 0; c < 6; ++c)
          CHECK(plan.records[6 * rpos + c] == E[c], "group %d record %zu coordinate %d", g, rpos, c);
      ++rpos;
      ++cnt;
    }
    CHECK(plan.off[g + 1] - plan.off[g] == cnt, "group %d: %d records, brute force %d", g, plan.off[g + 1] - plan.off[g],
          cnt);
    CHECK(plan.groups[g].num_corr == off[g + 1] - off[g], "group %d: num_corr", g);
    CHECK(plan.groups[g].key == (off[g + 1] > off[g] ? corr[2 * off[g]] : 0), "group %d: key %d", g, plan.groups[g].key);
    CHECK(plan.groups[g].run == (cnt >= 4), "group %d: run %d with %d records", g, plan.groups[g].run, cnt);
    run += cnt >= 4;
    few += cnt < 4;
  }
  CHECK(rpos == plan.rec_corr.size() && plan.records.size() == 6 * rpos, "stray records");
  CHECK(plan.num_run == run, "num_run %d against %d", plan.num_run, run);
  CHECK(plan.H == 1024 && plan.S == 4 && plan.grid == 4 * (int64_t)n, "launch shape");
  std::printf("P %d, %d groups: %zu records of %zu correspondences, %d groups run, %d do not\n", P, n, rpos,
              corr.size() / 2, run, few);
}

void check_shape_and_rules() {
  Map map(40, 5);
  for (int p = 0; p < 40; ++p) {   // every point usable
    map.flags[p] = 0;
    for (int c = 0; c < 4; ++c) map.X[4 * p + c] = 1.0 + p + c;
  }
  const int32_t corr[10] = {7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  const int32_t off4[2] = {0, 4}, off3[2] = {0, 3}, off5[2] = {0, 5};
  sg_align_options o = defaults();
  sg::AlignPlan plan;
  sg::PlanAlign(&map.m, corr, off4, 1, &o, &plan);
  CHECK(plan.num_run == 1 && plan.groups[0].run == 1 && plan.groups[0].key == 7 && plan.off[1] == 4, "N = 4 runs");
  sg::PlanAlign(&map.m, corr, off3, 1, &o, &plan);
  CHECK(plan.num_run == 0 && plan.groups[0].run == 0 && plan.off[1] == 3, "N = 3 does not run");
  // the key is that of the first listed correspondence, also when it is no record
  map.flags[7] = 1 << SG_BAD_FEATURE;
  sg::PlanAlign(&map.m, corr, off5, 1, &o, &plan);
  CHECK(plan.groups[0].key == 7 && plan.off[1] == 4 && plan.rec_corr[0] == 1 && plan.groups[0].run == 1, "key of a non-record");
  map.flags[7] = 0;
  // the hypothesis count: rounded up to 256, capped at 2^20
  const int want[][2] = {{1, 256}, {256, 256}, {257, 512}, {1024, 1024}, {1 << 20, 1 << 20}, {(1 << 20) + 1, 1 << 20},
                         {0x7fffffff, 1 << 20}};
  for (const auto& w : want) {
    o.max_hypotheses = w[0];
    sg::PlanAlign(&map.m, corr, off4, 1, &o, &plan);
    CHECK(plan.H == w[1] && plan.S == w[1] / 256 && plan.grid == plan.S, "H for %d: %d", w[0], plan.H);
  }
  o = defaults();
  // n == 0: an empty plan, the lists are not read
  sg::PlanAlign(&map.m, nullptr, nullptr, 0, &o, &plan);
  CHECK(plan.off.size() == 1 && plan.groups.empty() && plan.num_run == 0 && plan.grid == 0, "n == 0");
  // empty groups only: nothing to read in corr
  const int32_t off0[3] = {0, 0, 0};
  sg::PlanAlign(&map.m, nullptr, off0, 2, &o, &plan);
  CHECK(plan.num_run == 0 && plan.off[2] == 0, "empty groups");

  // every SG_EINVAL rule
  CHECK(plan_code(nullptr, corr, off4, 1, &o) == SG_EINVAL, "null map");
  CHECK(plan_code(&map.m, corr, off4, 1, nullptr) == SG_EINVAL, "null options");
  CHECK(plan_code(&map.m, nullptr, off4, 1, &o) == SG_EINVAL, "null corr");
  CHECK(plan_code(&map.m, corr, nullptr, 1, &o) == SG_EINVAL, "null offsets");
  CHECK(plan_code(&map.m, corr, off4, -1, &o) == SG_EINVAL, "n < 0");
  const int32_t off_bad0[2] = {1, 4}, off_dec[3] = {0, 4, 3};
  CHECK(plan_code(&map.m, corr, off_bad0, 1, &o) == SG_EINVAL, "group_offset[0] != 0");
  CHECK(plan_code(&map.m, corr, off_dec, 2, &o) == SG_EINVAL, "decreasing offset");
  for (int bad : {-1, 40, 0x7fffffff}) {
    for (int side = 0; side < 2; ++side) {
      int32_t c2[10];
      for (int i = 0; i < 10; ++i) c2[i] = corr[i];
      c2[8 + side] = bad;   // the fifth correspondence
      CHECK(plan_code(&map.m, c2, off5, 1, &o) == SG_EINVAL, "index %d on side %d", bad, side);
      CHECK(plan_code(&map.m, c2, off4, 1, &o) == SG_OK, "a correspondence beyond the listed ones is not read");
    }
  }
  int32_t same[10];
  for (int i = 0; i < 10; ++i) same[i] = corr[i];
  same[3] = same[2];
  CHECK(plan_code(&map.m, same, off4, 1, &o) == SG_EINVAL, "a == b");
  struct Bad {
    double threshold;
    int32_t hyp;
    double min_gap, max_scale;
  };
  const Bad bads[] = {{0.0, 1024, 1e-6, 0.0},  {-1.0, 1024, 1e-6, 0.0}, {kNaN, 1024, 1e-6, 0.0}, {10.0, 0, 1e-6, 0.0},
                      {10.0, -256, 1e-6, 0.0}, {10.0, 1024, -1e-9, 0.0}, {10.0, 1024, kNaN, 0.0}, {10.0, 1024, 1e-6, 0.5},
                      {10.0, 1024, 1e-6, -2.0}, {10.0, 1024, 1e-6, kNaN}};
  for (const Bad& b : bads) {
    sg_align_options x = defaults();
    x.threshold = b.threshold;
    x.max_hypotheses = b.hyp;
    x.min_gap = b.min_gap;
    x.max_scale = b.max_scale;
    CHECK(plan_code(&map.m, corr, off4, 1, &x) == SG_EINVAL, "options %g %d %g %g", b.threshold, b.hyp, b.min_gap,
          b.max_scale);
    CHECK(plan_code(&map.m, nullptr, nullptr, 0, &x) == SG_EINVAL, "options %g %d %g %g with n == 0", b.threshold, b.hyp,
          b.min_gap, b.max_scale);
  }
  for (double ok : {1.0, 1.5, 1e9}) {
    sg_align_options x = defaults();
    x.max_scale = ok;
    x.min_gap = 0.0;
    CHECK(plan_code(&map.m, corr, off4, 1, &x) == SG_OK, "max_scale %g", ok);
  }
  // too many groups for the hypothesis count: n * S must fit the grid
  std::vector<int32_t> many(4097, 0);
  sg_align_options x = defaults();
  x.max_hypotheses = 1 << 20;
  CHECK(plan_code(&map.m, nullptr, many.data(), 4096, &x) == SG_OK, "the grid is not reached for 4096 empty groups");
  std::vector<int32_t> more((1 << 19) + 1, 0);
  CHECK(plan_code(&map.m, nullptr, more.data(), 1 << 19, &x) == SG_EINVAL, "grid overflow");
}

}  // namespace

int main() {
  check_records(60, 6, 1);
  check_records(500, 12, 2);
  check_records(17, 40, 3);
  check_shape_and_rules();
  if (g_fail) {
    std::printf("align_plan_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("align_plan_check OK\n");
  return 0;
}
