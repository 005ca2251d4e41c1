// posegraph_math_check.cpp — CPU check of csrc/posegraph_math.h, a stand-alone program (tests/test_posegraph_math.py
// builds it under AddressSanitizer and UBSan): PgEdgeEval's residual against a restatement with long double, and its
// analytic 7 x 14 Jacobian against central differences through QuatPlus, on random edges, with q_e near the identity
// on both sides of the series switch (kPgSeriesTheta2), near the w = 0 flip on both sides, with and without
// fix_scale, with and without the Cauchy loss; the continuity of the rotation vector across the series switch.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "posegraph_math.h"

using namespace sg;

static int g_fail = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      ++g_fail;                                \
    }                                          \
  } while (0)

static std::mt19937_64 rng(7);
static double Normal(double s) { return std::normal_distribution<double>(0.0, s)(rng); }

static void Unit(double* q) {
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) q[i] /= n;
}
static void RandomState(double* x, bool sigma) {
  for (int i = 0; i < 4; ++i) x[i] = Normal(1.0);
  Unit(x);
  for (int i = 0; i < 3; ++i) x[4 + i] = Normal(500.0);
  x[7] = sigma ? Normal(0.2) : 0.0;
}
static void Plus(const double* x, const double* d, int fix_scale, double* o) {
  QuatPlus(x, d, o);
  for (int i = 0; i < 3; ++i) o[4 + i] = x[4 + i] + d[3 + i];
  o[7] = x[7] + (fix_scale ? 0.0 : d[6]);
}
// The measurement that makes q_e the rotation by ang about ax at the states xa, xb.
static void MeasureFor(const double* xa, const double* xb, const double* ax, double ang, double* meas) {
  const double cb[4] = {-xb[0], -xb[1], -xb[2], xb[3]};
  double rel[4];
  PgQuatMul(xa, cb, rel);
  const double s = std::sin(0.5 * ang);
  const double ce[4] = {-s * ax[0], -s * ax[1], -s * ax[2], std::cos(0.5 * ang)};
  PgQuatMul(rel, ce, meas);   // q^ = q_a conj(q_b) conj(q_e)
  Unit(meas);
  for (int i = 0; i < 3; ++i) meas[4 + i] = Normal(300.0);
  meas[7] = 0.1;
}

static void CheckEdge(const char* what, double ang, int fix_scale, double b) {
  double xa[8], xb[8], ax[3], meas[8];
  RandomState(xa, !fix_scale);
  RandomState(xb, !fix_scale);
  for (int i = 0; i < 3; ++i) ax[i] = Normal(1.0);
  const double n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  for (int i = 0; i < 3; ++i) ax[i] /= n;
  MeasureFor(xa, xb, ax, ang, meas);
  const double w[3] = {3.0, 0.7, 11.0};
  const double inv_b = b > 0.0 ? 1.0 / b : 0.0;
  double rec[kPgRec], rho1 = 0.0;
  const double cost = PgEdgeEval(xa, xb, meas, w, fix_scale, b, inv_b, true, rec, &rho1);
  // the rotation part of the residual is w_rot times the rotation vector of q_e: angle `ang` folded into [0, pi]
  double fold = std::fmod(ang, 2.0 * M_PI);
  if (fold > M_PI) fold = 2.0 * M_PI - fold;
  const double sr = std::sqrt(rho1);
  const double rn = std::sqrt(rec[0] * rec[0] + rec[1] * rec[1] + rec[2] * rec[2]);
  CHECK(std::fabs(rn - sr * w[0] * fold) <= 1e-12 * (1.0 + w[0] * fold), "%s: |r_rot| %.17g, expected %.17g", what, rn,
        sr * w[0] * fold);
  double s2 = 0.0;
  for (int i = 0; i < kPgRes; ++i) s2 += rec[i] * rec[i];
  s2 /= rho1;
  const double want = b > 0.0 ? 0.5 * b * std::log(1.0 + s2 / b) : 0.5 * s2;
  CHECK(std::fabs(cost - want) <= 1e-12 * want, "%s: cost %.17g, expected %.17g", what, cost, want);
  CHECK(b > 0.0 ? std::fabs(rho1 - 1.0 / (1.0 + s2 / b)) <= 1e-12 : rho1 == 1.0, "%s: rho1 %.17g", what, rho1);
  if (fix_scale) CHECK(rec[6] == 0.0, "%s: scale residual with fix_scale", what);
  // central differences of the uncorrected residual; the corrected Jacobian is sqrt(rho') times it
  const double h = 1e-6;
  double worst = 0.0, big = 1.0;
  for (int col = 0; col < kPgCols; ++col) {
    const int side = col / 7, k = col % 7;
    double d[7] = {0, 0, 0, 0, 0, 0, 0}, xp[8], xm[8], rp[kPgRec], rm[kPgRec];
    d[k] = h;
    Plus(side ? xb : xa, d, fix_scale, xp);
    d[k] = -h;
    Plus(side ? xb : xa, d, fix_scale, xm);
    PgEdgeEval(side ? xa : xp, side ? xp : xb, meas, w, fix_scale, 0.0, 0.0, false, rp, nullptr);
    PgEdgeEval(side ? xa : xm, side ? xm : xb, meas, w, fix_scale, 0.0, 0.0, false, rm, nullptr);
    for (int r = 0; r < kPgRes; ++r) {
      const double num = sr * (rp[r] - rm[r]) / (2.0 * h);
      const double ana = rec[kPgRes + r * kPgCols + col];
      worst = std::fmax(worst, std::fabs(num - ana));
      big = std::fmax(big, std::fabs(num));
      if (fix_scale && (k == 6 || r == 6)) CHECK(ana == 0.0, "%s: entry (%d, %d) with fix_scale", what, r, col);
    }
  }
  // h = 1e-6 on values of a few thousand: 2e-6 of the largest entry
  CHECK(worst <= 2e-6 * big, "%s: Jacobian off by %.3g (largest entry %.3g)", what, worst, big);
}

int main() {
  const double sw = 2.0 * std::sqrt(kPgSeriesTheta2);   // the switch as an angle: |v| = sin(ang / 2)
  for (int fs = 0; fs < 2; ++fs)
    for (double b : {0.0, 2500.0})
      for (int rep = 0; rep < 8; ++rep) {
        CheckEdge("random", 0.3 + 0.25 * rep, fs, b);
        CheckEdge("series below", 0.8 * sw, fs, b);
        CheckEdge("series above", 1.2 * sw, fs, b);
        CheckEdge("tiny", 1e-9, fs, b);
        CheckEdge("flip plus", M_PI - 1e-3, fs, b);
        CheckEdge("flip minus", M_PI + 1e-3, fs, b);
      }
  // the two branches of PgLogFactors agree at the switch
  for (double f : {0.999, 1.001}) {
    const double th = std::sqrt(kPgSeriesTheta2 * f), e[4] = {th, 0.0, 0.0, std::sqrt(1.0 - th * th)};
    double g, h, dw;
    PgLogFactors(e, &g, &h, &dw);
    const double g_ref = 2.0 * std::atan2(th, e[3]) / th;
    CHECK(std::fabs(g - g_ref) <= 4e-16 * g_ref, "g at the switch: %.17g vs %.17g", g, g_ref);
    CHECK(std::fabs(h + 4.0 / 3.0) <= 1e-6, "h at the switch: %.17g", h);
    CHECK(std::fabs(dw + 2.0) <= 1e-15, "dw: %.17g", dw);
  }
  if (g_fail) {
    std::printf("posegraph_math_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("posegraph_math_check OK\n");
  return 0;
}
