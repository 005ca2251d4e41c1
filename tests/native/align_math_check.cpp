// CPU check of csrc/align_math.h on a case file written by tests/test_align_math.py from the numpy references
// (argv[1]): AlignHorn on three records and on all records of the scenes against numpy's Horn (rotation from an SVD,
// gap from eigh), fix_scale giving a scale of exactly 1, the residual against numpy; then, built here: a mirrored copy
// gives a proper rotation with a large residual, and collinear, coincident, NaN, zero-spread and out-of-gate inputs
// give no model.  Built under AddressSanitizer and UBSan by that test.  No GPU, no HIP.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "align_math.h"

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

bool read(FILE* f, double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (std::fscanf(f, "%lf", &v[i]) != 1) return false;
  return true;
}

double det3(const double* R) {
  return R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
}

// One case: n, fix_scale, k | records [6 n] | k indices | s, q[4], t[3], gap of numpy | tolerances: q, t, log s, gap |
// a generic transform s, R[9], t[3] | its e^2 per record [n].
bool check_case(FILE* f, int ci, std::vector<double>* first_records) {
  double head[3];
  if (!read(f, head, 3)) return false;
  const int n = (int)head[0], fix = (int)head[1], k = (int)head[2];
  std::vector<double> rec(6 * (size_t)n), idx(k), e2(n);
  double ref[9], tol[4], G[13];
  if (!read(f, rec.data(), 6 * n) || !read(f, idx.data(), k) || !read(f, ref, 9) || !read(f, tol, 4) ||
      !read(f, G, 13) || !read(f, e2.data(), n))
    return false;
  if (ci == 0) *first_records = rec;
  std::vector<double> sel(6 * (size_t)k);
  for (int j = 0; j < k; ++j)
    for (int c = 0; c < 6; ++c) sel[6 * (size_t)j + c] = rec[6 * (size_t)idx[j] + c];
  sg::AlignXf xf{};
  double gap = -1.0;
  const bool ok = sg::AlignHorn(sel.data(), k, fix, 0.0, &xf, &gap);
  CHECK(ok, "case %d: no model", ci);
  if (!ok) return true;
  double dq = 0.0, dt = 0.0;
  for (int i = 0; i < 4; ++i) dq = std::fmax(dq, std::fabs(xf.q[i] - ref[1 + i]));
  for (int i = 0; i < 3; ++i) dt = std::fmax(dt, std::fabs(xf.t[i] - ref[5 + i]));
  const double qn = std::sqrt(xf.q[0] * xf.q[0] + xf.q[1] * xf.q[1] + xf.q[2] * xf.q[2] + xf.q[3] * xf.q[3]);
  std::printf("case %d: n %d of %d, fix %d, gap %.6f, |dq| %.3e (tol %.3e), |dt| %.3e (tol %.3e), dlog s %.3e\n", ci, k,
              n, fix, gap, dq, tol[0], dt, tol[1], std::fabs(std::log(xf.s / ref[0])));
  CHECK(dq <= tol[0], "case %d: q off by %.3e", ci, dq);
  CHECK(dt <= tol[1], "case %d: t off by %.3e", ci, dt);
  CHECK(std::fabs(std::log(xf.s / ref[0])) <= tol[2], "case %d: scale %.17g against %.17g", ci, xf.s, ref[0]);
  CHECK(std::fabs(gap - ref[8]) <= tol[3], "case %d: gap %.17g against %.17g", ci, gap, ref[8]);
  CHECK(std::fabs(qn - 1.0) < 1e-14 && xf.q[3] >= 0.0, "case %d: q not unit with w >= 0", ci);
  if (fix) CHECK(xf.s == 1.0, "case %d: fix_scale gave %.17g", ci, xf.s);
  double A[9];
  sg::AlignMatrix(G[0], xf.q, A);   // (only to exercise AlignMatrix on a unit q: its determinant is s^3)
  CHECK(std::fabs(det3(A) / (G[0] * G[0] * G[0]) - 1.0) < 1e-13, "case %d: det of s R", ci);
  // the residual against numpy, at the generic transform (its matrix is given, scaled here)
  double GA[9];
  for (int i = 0; i < 9; ++i) GA[i] = G[0] * G[1 + i];
  for (int i = 0; i < n; ++i) {
    const double r2 = sg::AlignResidual2(GA, G + 10, &rec[6 * (size_t)i], &rec[6 * (size_t)i + 3]);
    CHECK(std::fabs(r2 - e2[i]) <= 1e-12 * e2[i], "case %d record %d: e2 %.17g against %.17g", ci, i, r2, e2[i]);
  }
  return true;
}

void check_no_model(const std::vector<double>& base) {
  const int n = (int)(base.size() / 6);
  sg::AlignXf xf{};
  double gap;
  // a mirrored copy: Horn still returns a proper rotation, which cannot fit
  std::vector<double> rec = base;
  for (int i = 0; i < n; ++i) {
    rec[6 * i + 3] = -base[6 * i];
    rec[6 * i + 4] = base[6 * i + 1];
    rec[6 * i + 5] = base[6 * i + 2];
  }
  bool ok = sg::AlignHorn(rec.data(), n, 0, 0.0, &xf, &gap);
  CHECK(ok, "mirrored copy: no model");
  if (ok) {
    double A[9], worst = 0.0;
    sg::AlignMatrix(1.0, xf.q, A);
    CHECK(std::fabs(det3(A) - 1.0) < 1e-13, "mirrored copy: det %.17g", det3(A));
    sg::AlignMatrix(xf.s, xf.q, A);
    for (int i = 0; i < n; ++i) worst = std::fmax(worst, sg::AlignResidual2(A, xf.t, &rec[6 * i], &rec[6 * i + 3]));
    std::printf("mirrored copy: det +1, worst residual %.1f\n", std::sqrt(worst));
    CHECK(worst > 100.0 * 100.0, "mirrored copy fits: %.3e", worst);
  }
  // three collinear records (Y = 2 X + 1)
  double col[18];
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 3; ++c) {
      col[6 * i + c] = 100.0 + (i * i + 1) * (c + 1) * 37.0;
      col[6 * i + 3 + c] = 2.0 * col[6 * i + c] + 1.0;
    }
  CHECK(!sg::AlignHorn(col, 3, 0, 0.0, &xf, &gap) && gap <= sg::kAlignMinGap, "collinear sample gave a model, gap %.3e",
        gap);
  // coincident records on the a side: zero spread
  double same[18];
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 3; ++c) {
      same[6 * i + c] = 5.0 + c;
      same[6 * i + 3 + c] = base[6 * i + 3 + c];
    }
  CHECK(!sg::AlignHorn(same, 3, 0, 0.0, &xf, &gap), "zero spread in a gave a model");
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 3; ++c) {
      same[6 * i + c] = base[6 * i + c];
      same[6 * i + 3 + c] = 7.0 - c;
    }
  CHECK(!sg::AlignHorn(same, 3, 0, 0.0, &xf, &gap), "zero spread in b gave a model");
  CHECK(!sg::AlignHorn(same, 3, 1, 0.0, &xf, &gap), "zero spread in b gave a model with fix_scale");
  // all three records the same
  for (int i = 0; i < 18; ++i) same[i] = base[i % 6];
  CHECK(!sg::AlignHorn(same, 3, 0, 0.0, &xf, &gap), "coincident records gave a model");
  // NaN and infinity
  for (int bad = 0; bad < 18; ++bad) {
    double r3[18];
    for (int i = 0; i < 18; ++i) r3[i] = base[i];
    r3[bad] = std::numeric_limits<double>::quiet_NaN();
    CHECK(!sg::AlignHorn(r3, 3, 0, 0.0, &xf, &gap) && gap == 0.0, "NaN at %d gave a model", bad);
    r3[bad] = std::numeric_limits<double>::infinity();
    CHECK(!sg::AlignHorn(r3, 3, 0, 0.0, &xf, &gap) && gap == 0.0, "infinity at %d gave a model", bad);
  }
  // the scale gate: Y = 1.3 R X + t has a model without a gate and inside it, none outside; fix_scale passes any gate
  CHECK(sg::AlignHorn(base.data(), 3, 0, 0.0, &xf, &gap), "no model without a gate");
  const double s = xf.s;
  CHECK(sg::AlignHorn(base.data(), 3, 0, 2.0, &xf, &gap) && xf.s == s, "no model inside the gate");
  CHECK(!sg::AlignHorn(base.data(), 3, 0, 1.1, &xf, &gap), "a model outside the gate (scale %.3f)", s);
  CHECK(sg::AlignHorn(base.data(), 3, 1, 1.0, &xf, &gap) && xf.s == 1.0, "fix_scale inside a gate of 1");
  // the gate from below: the inverse direction has the scale 1 / 1.3
  std::vector<double> inv = base;
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 3; ++c) {
      inv[6 * i + c] = base[6 * i + 3 + c];
      inv[6 * i + 3 + c] = base[6 * i + c];
    }
  CHECK(sg::AlignHorn(inv.data(), 3, 0, 2.0, &xf, &gap) && std::fabs(xf.s * s - 1.0) < 1e-12, "inverse inside the gate");
  CHECK(!sg::AlignHorn(inv.data(), 3, 0, 1.1, &xf, &gap), "inverse outside the gate");
  // the status rule
  CHECK(sg::AlignStatus(3, 1.0, 0, 1e-6) == SG_ALIGN_FEW_INLIERS && sg::AlignStatus(7, 1.0, 8, 1e-6) == SG_ALIGN_FEW_INLIERS,
        "few inliers");
  CHECK(sg::AlignStatus(8, 1e-7, 8, 1e-6) == SG_ALIGN_DEGENERATE && sg::AlignStatus(8, 1e-6, 8, 1e-6) == SG_ALIGN_OK &&
            sg::AlignStatus(4, 0.0, 0, 0.0) == SG_ALIGN_OK,
        "gap rule");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: align_math_check cases.txt\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::printf("cannot open %s\n", argv[1]);
    return 2;
  }
  double nc;
  if (!read(f, &nc, 1)) return 2;
  std::vector<double> first;
  for (int ci = 0; ci < (int)nc; ++ci)
    if (!check_case(f, ci, &first)) {
      std::printf("case file ends early at case %d\n", ci);
      return 2;
    }
  std::fclose(f);
  if (first.size() < 18) return 2;
  check_no_model(first);
  if (g_fail) {
    std::printf("align_math_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("align_math_check OK (%d cases)\n", (int)nc);
  return 0;
}
