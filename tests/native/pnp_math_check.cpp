// CPU check of csrc/pnp_math.h (the one copy k_pose_ransac and k_pose_select run): the sampler against a table the
// numpy restatement (tests/localize_cases.py, sample_np) printed; P3P on generated exact configurations; degenerate
// samples; the quaternion's sign and norm; the score's rules.  Built under AddressSanitizer and UBSan by
// tests/test_localize_math.py.  No GPU, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "pnp_math.h"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                           \
  do {                                             \
    if (!(cond)) {                                 \
      if (++g_fail <= 20) {                        \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                  \
        std::printf("\n");                         \
      }                                            \
    }                                              \
  } while (0)

struct Rng {   // 64-bit LCG (Knuth's MMIX constants), top 53 bits
  uint64_t s;
  double uni() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) * (1.0 / 9007199254740992.0);
  }
  double uni(double a, double b) { return a + (b - a) * uni(); }
};

void quat_rotate(const double* q, const double* v, double* p) {
  const double zero[3] = {0, 0, 0}, X[4] = {v[0], v[1], v[2], 1.0};
  double vv[3];
  sg::CameraPoint(q, zero, X, vv, p);
}

// ------------------------------------------------------------------------------------------------ sampler
struct SampleRow {
  uint32_t seed;
  int32_t f, n;
  int32_t idx[6][3];   // h = 0, 1, 2, 255, 256, 1023
};
const SampleRow kTable[] = {
    {0u, 8, 4, {{2, 1, 0}, {2, 0, 1}, {0, 1, 2}, {2, 0, 3}, {0, 3, 1}, {3, 2, 1}}},
    {0u, 8, 5, {{3, 1, 0}, {3, 0, 2}, {1, 0, 2}, {2, 0, 4}, {0, 3, 2}, {4, 3, 2}}},
    {7u, 3, 64, {{45, 20, 13}, {32, 40, 14}, {5, 24, 44}, {32, 39, 1}, {40, 55, 7}, {39, 8, 52}}},
    {3735928559u, 123456, 1025,
     {{590, 348, 807}, {293, 8, 114}, {563, 598, 554}, {527, 796, 905}, {113, 178, 752}, {683, 598, 307}}},
};
const int kTableH[6] = {0, 1, 2, 255, 256, 1023};

void check_sampler() {
  for (const SampleRow& row : kTable)
    for (int j = 0; j < 6; ++j) {
      int32_t idx[3];
      sg::PnpSample(row.seed, row.f, kTableH[j], row.n, idx);
      CHECK(idx[0] == row.idx[j][0] && idx[1] == row.idx[j][1] && idx[2] == row.idx[j][2],
            "sampler table n %d h %d: %d %d %d", row.n, kTableH[j], idx[0], idx[1], idx[2]);
    }
  const int ns[4] = {4, 5, 64, 1025};
  for (int n : ns) {
    long hits[4] = {0, 0, 0, 0};
    for (uint32_t seed = 0; seed < 3; ++seed)
      for (int f = 0; f < 3; ++f)
        for (int h = 0; h < 4096; ++h) {
          int32_t idx[3];
          sg::PnpSample(seed, f, h, n, idx);
          bool ok = true;
          for (int j = 0; j < 3; ++j) ok = ok && idx[j] >= 0 && idx[j] < n;
          ok = ok && idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2];
          CHECK(ok, "sample n %d seed %u f %d h %d: %d %d %d", n, seed, f, h, idx[0], idx[1], idx[2]);
          if (n == 4 && ok)
            for (int j = 0; j < 3; ++j) hits[idx[j]]++;
        }
    if (n == 4)   // every index is drawn: 3/4 of 3 * 3 * 4096 draws each, within 5 %
      for (int i = 0; i < 4; ++i)
        CHECK(std::fabs(hits[i] / 27648.0 - 1.0) < 0.05, "index %d drawn %ld times", i, hits[i]);
  }
}

// ------------------------------------------------------------------------------------------------ P3P
// A random pose and three points in front of it, in the robot's ranges: depths 1000 .. 6000, bearings inside the
// 640 x 480 image at focal length 416, any two at least 0.05 rad apart.
struct Config {
  double q[4], t[3], f[3][3], P[3][3];
};

Config make_config(Rng& r) {
  Config c;
  double n2 = 0.0;
  for (int i = 0; i < 4; ++i) {
    c.q[i] = r.uni(-1.0, 1.0);
    n2 += c.q[i] * c.q[i];
  }
  const double inv = (c.q[3] < 0 ? -1.0 : 1.0) / std::sqrt(n2);
  for (int i = 0; i < 4; ++i) c.q[i] *= inv;
  for (int i = 0; i < 3; ++i) c.t[i] = r.uni(-5000.0, 5000.0);
  const double qc[4] = {-c.q[0], -c.q[1], -c.q[2], c.q[3]};   // camera -> world
  for (;;) {
    for (int j = 0; j < 3; ++j) {
      const double a = r.uni(-320.0, 320.0) / 416.0, b = r.uni(-240.0, 240.0) / 416.0;
      const double s = 1.0 / std::sqrt(a * a + b * b + 1.0);
      c.f[j][0] = a * s;
      c.f[j][1] = b * s;
      c.f[j][2] = s;
    }
    bool apart = true;
    for (int i = 0; i < 3; ++i)
      for (int j = i + 1; j < 3; ++j) apart = apart && sg::pnp_cross2(c.f[i], c.f[j]) > 0.05 * 0.05;
    // and not close to one line in the image (the triangle's area in the plane z = 1)
    const double ax = c.f[1][0] / c.f[1][2] - c.f[0][0] / c.f[0][2], ay = c.f[1][1] / c.f[1][2] - c.f[0][1] / c.f[0][2];
    const double bx = c.f[2][0] / c.f[2][2] - c.f[0][0] / c.f[0][2], by = c.f[2][1] / c.f[2][2] - c.f[0][1] / c.f[0][2];
    if (apart && std::fabs(ax * by - ay * bx) > 0.02) break;
  }
  for (int j = 0; j < 3; ++j) {
    const double d = r.uni(1000.0, 6000.0);
    const double y[3] = {d * c.f[j][0], d * c.f[j][1], d * c.f[j][2]};
    double w[3];
    quat_rotate(qc, y, w);
    for (int i = 0; i < 3; ++i) c.P[j][i] = w[i] + c.t[i];
  }
  return c;
}

void check_p3p() {
  Rng r{12345};
  const int kConfigs = 4000;
  int found = 0, roots_total = 0, poses_total = 0;
  double worst_reproj = 0.0, worst_q = 0.0, worst_t = 0.0;
  for (int n = 0; n < kConfigs; ++n) {
    const Config c = make_config(r);
    sg::P3pProblem pr;
    const bool ok = sg::P3pSetup(c.f, c.P, &pr);
    CHECK(ok, "config %d: setup refused", n);
    if (!ok) continue;
    double v[4];
    const int nr = sg::P3pQuartic(pr, v);
    CHECK(nr >= 0 && nr <= 4, "config %d: %d roots", n, nr);
    roots_total += nr;
    double best_q = 1e300, best_t = 1e300;
    for (int i = 0; i < nr; ++i) {
      double q[4], t[3];
      if (!sg::P3pPose(c.f, c.P, pr, v[i], q, t)) continue;
      ++poses_total;
      // the quaternion's norm and sign
      const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      CHECK(std::fabs(qn - 1.0) < 1e-14 && q[3] >= 0.0, "config %d root %d: |q| - 1 = %.3e, w = %.3e", n, i, qn - 1.0,
            q[3]);
      // every returned pose reprojects its three points: the sine of the angle to the bearing
      for (int j = 0; j < 3; ++j) {
        const double d[3] = {c.P[j][0] - t[0], c.P[j][1] - t[1], c.P[j][2] - t[2]};
        double p[3];
        quat_rotate(q, d, p);
        CHECK(sg::pnp_dot(p, c.f[j]) > 0.0, "config %d root %d: point %d behind the camera", n, i, j);
        const double s = std::sqrt(sg::pnp_cross2(p, c.f[j]) / sg::pnp_dot(p, p));
        if (s > worst_reproj) worst_reproj = s;
        CHECK(s < 1e-9, "config %d root %d point %d: sine %.3e", n, i, j, s);
      }
      double dq = 0.0, dt = 0.0;
      for (int j = 0; j < 4; ++j) dq = std::fmax(dq, std::fabs(q[j] - c.q[j]));
      for (int j = 0; j < 3; ++j) dt = std::fmax(dt, std::fabs(t[j] - c.t[j]));
      if (dq + dt * 1e-4 < best_q + best_t * 1e-4) {
        best_q = dq;
        best_t = dt;
      }
    }
    // the true pose is among the roots: rotation 1e-8, centre 1e-4 map units (1e-8 of the scene's 1e4)
    const bool hit = best_q < 1e-8 && best_t < 1e-4;
    CHECK(hit, "config %d: true pose not among %d roots (q %.3e, t %.3e)", n, nr, best_q, best_t);
    if (hit) {
      ++found;
      worst_q = std::fmax(worst_q, best_q);
      worst_t = std::fmax(worst_t, best_t);
    }
  }
  std::printf("p3p: %d configs, true pose found in %d, %d roots, %d poses; worst sine %.3e, q %.3e, t %.3e\n", kConfigs,
              found, roots_total, poses_total, worst_reproj, worst_q, worst_t);
}

void expect_no_pose(const char* what, const double (*f)[3], const double (*P)[3]) {
  sg::P3pProblem pr;
  int poses = 0;
  if (sg::P3pSetup(f, P, &pr)) {
    double v[4];
    const int nr = sg::P3pQuartic(pr, v);
    for (int i = 0; i < nr; ++i) {
      double q[4], t[3];
      if (sg::P3pPose(f, P, pr, v[i], q, t)) {
        ++poses;
        for (int j = 0; j < 4; ++j) CHECK(sg::PnpFinite(q[j]), "%s: non-finite q", what);
        for (int j = 0; j < 3; ++j) CHECK(sg::PnpFinite(t[j]), "%s: non-finite t", what);
      }
    }
  }
  CHECK(poses == 0, "%s: %d poses", what, poses);
}

void check_degenerate() {
  Rng r{777};
  for (int n = 0; n < 200; ++n) {
    Config c = make_config(r);
    // collinear points: the third on the line through the first two
    Config a = c;
    const double s = r.uni(-2.0, 3.0);
    for (int i = 0; i < 3; ++i) a.P[2][i] = a.P[0][i] + s * (a.P[1][i] - a.P[0][i]);
    expect_no_pose("collinear points", a.f, a.P);
    // two equal points
    Config b = c;
    for (int i = 0; i < 3; ++i) b.P[1][i] = b.P[0][i];
    expect_no_pose("two equal points", b.f, b.P);
    // two equal bearings
    Config d = c;
    for (int i = 0; i < 3; ++i) d.f[2][i] = d.f[0][i];
    expect_no_pose("two equal bearings", d.f, d.P);
    // a non-finite point or bearing
    Config e = c;
    e.P[1][1] = NAN;
    expect_no_pose("NaN point", e.f, e.P);
    Config g = c;
    g.f[0][2] = INFINITY;
    expect_no_pose("infinite bearing", g.f, g.P);
  }
  // |X.w| under the limit, zero, NaN: no Euclidean point
  double P[3];
  const double far[4] = {0.6, 0.0, 0.8, 0.5e-9}, zero[4] = {0.6, 0.0, 0.8, 0.0}, nan[4] = {0.6, 0.0, 0.8, NAN};
  const double neg[4] = {0.6, 0.0, 0.8, -0.5e-9}, fine[4] = {0.3, 0.0, 0.4, -0.5};
  CHECK(!sg::PnpEuclidean(far, P) && !sg::PnpEuclidean(zero, P) && !sg::PnpEuclidean(nan, P) &&
            !sg::PnpEuclidean(neg, P),
        "w under the limit accepted");
  CHECK(sg::PnpEuclidean(fine, P) && P[0] == -0.6 && P[1] == 0.0 && P[2] == -0.8, "Euclidean point");
}

// ------------------------------------------------------------------------------------------------ quaternion, score
void check_quaternion() {
  Rng r{99};
  for (int n = 0; n < 4000; ++n) {
    double q[4], n2 = 0.0;
    for (int i = 0; i < 4; ++i) {
      q[i] = r.uni(-1.0, 1.0);
      n2 += q[i] * q[i];
    }
    if (n % 4 == 1) q[3] *= 1e-3;   // small w: the three diagonal branches
    if (n % 4 == 2) q[3] = 0.0;
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const double inv = 1.0 / std::sqrt(n2);
    for (int i = 0; i < 4; ++i) q[i] *= inv;
    double R[9];
    for (int c = 0; c < 3; ++c) {
      double e[3] = {0, 0, 0}, p[3];
      e[c] = 1.0;
      quat_rotate(q, e, p);
      for (int i = 0; i < 3; ++i) R[3 * i + c] = p[i];
    }
    double o[4];
    sg::PnpQuatFromRotation(R, o);
    const double on = std::sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
    CHECK(std::fabs(on - 1.0) < 1e-15 * 4 && o[3] >= 0.0, "quaternion %d: norm %.3e, w %.3e", n, on - 1.0, o[3]);
    // the same rotation: o = +-q
    double dp = 0.0, dm = 0.0;
    for (int i = 0; i < 4; ++i) {
      dp = std::fmax(dp, std::fabs(o[i] - q[i]));
      dm = std::fmax(dm, std::fabs(o[i] + q[i]));
    }
    CHECK(std::fmin(dp, dm) < 1e-12, "quaternion %d: off by %.3e", n, std::fmin(dp, dm));
  }
}

void check_score_and_bearing() {
  const double k[7] = {-0.1, 0.02, -0.001, 416.0, -416.0, 320.0, 240.0};
  const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
  const double X[4] = {100.0 / 2000.0, -50.0 / 2000.0, 1000.0 / 2000.0, 1.0 / 2000.0};
  double uv[2];
  CHECK(sg::Project(q, t, k, X, uv), "projection refused");
  // the bearing of the projected pixel points at the point
  double f[3];
  sg::PnpBearing(k, uv, f);
  const double P[3] = {100.0, -50.0, 1000.0};
  CHECK(std::sqrt(sg::pnp_cross2(f, P) / sg::pnp_dot(P, P)) < 1e-14, "bearing off");
  CHECK(std::fabs(sg::pnp_dot(f, f) - 1.0) < 1e-15, "bearing not unit");
  int in = 7;
  const double pt3[2] = {uv[0] + 3.0, uv[1]}, pt4[2] = {uv[0], uv[1] - 4.0}, pt5[2] = {uv[0] + 3.0, uv[1] + 4.0};
  CHECK(std::fabs(sg::PnpScore(q, t, k, X, pt3, 16.0, &in) - 9.0) < 1e-9 && in == 1, "3 px inside 4");
  CHECK(sg::PnpScore(q, t, k, X, pt4, 16.0, &in) <= 16.0 && in == 1, "4 px counts as an inlier of 4");
  CHECK(sg::PnpScore(q, t, k, X, pt5, 16.0, &in) == 16.0 && in == 0, "5 px is truncated");
  const double nanpt[2] = {NAN, 0.0};
  CHECK(sg::PnpScore(q, t, k, X, nanpt, 16.0, &in) == 16.0 && in == 0, "NaN pixel");
  const double behind[4] = {X[0], X[1], -X[2], X[3]};
  CHECK(sg::PnpScore(q, t, k, behind, uv, 16.0, &in) == 16.0 && in == 0, "behind the camera");
  const double qn[4] = {NAN, 0, 0, 1};
  CHECK(sg::PnpScore(qn, t, k, X, uv, 16.0, &in) == 16.0 && in == 0, "NaN pose");
}

}  // namespace

int main() {
  check_sampler();
  check_p3p();
  check_degenerate();
  check_quaternion();
  check_score_and_bearing();
  if (g_fail) {
    std::printf("pnp_math_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("pnp_math_check OK\n");
  return 0;
}
