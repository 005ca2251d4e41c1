// triangulate_math_check.cpp — CPU check of the per-point arithmetic of sg_slam_triangulate_points
// (slam-robot_amd/csrc/triangulate_math.h, the one copy k_point_triangulate runs):
//   - TriJacobi4 on generated symmetric 4x4 matrices (random symmetric, A^T A of rank 4, 3 and 1, repeated
//     eigenvalues, diagonal, zero, scaled over 1e-8 .. 1e8): |M v - l v| <= 64 eps |M|_F, |v| = 1, l the smallest
//     eigenvalue (M - l I is positive semi-definite up to rounding, and no sampled Rayleigh quotient is below l),
//     the eigenvalues ascending with the trace of M as their sum;
//   - UndistortPixel: every pixel of the 640x480 image through the inverse and the forward model again, within
//     1e-9 px, for k = (-0.1, 0.02, 0) and for k = 0;
//   - TriangulatePoint on hand-built cases: an exact two-view point and one case per status.
// Built stand-alone with -fsanitize=address,undefined by tests/test_triangulate_math.py.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "triangulate_math.h"

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
  double unit() { return next() / 2147483648.0; }
  double sym() { return 2.0 * unit() - 1.0; }
};

static const double kEps = DBL_EPSILON;

struct Sym4 {
  double a[4][4];
  void upper(double* M) const {
    int e = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = i; j < 4; ++j) M[e++] = a[i][j];
  }
};

static Sym4 Gram(const std::vector<double>& A, int rows) {   // A^T A, A row-major rows x 4
  Sym4 s{};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double v = 0.0;
      for (int r = 0; r < rows; ++r) v += A[4 * r + i] * A[4 * r + j];
      s.a[i][j] = v;
    }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < i; ++j) s.a[i][j] = s.a[j][i];
  return s;
}

// Q diag(d) Q^T with Q a Householder reflection
static Sym4 FromSpectrum(Rng& rng, const double* d) {
  double u[4], n = 0.0;
  for (int i = 0; i < 4; ++i) {
    u[i] = rng.sym();
    n += u[i] * u[i];
  }
  n = std::sqrt(n);
  double Q[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) Q[i][j] = (i == j ? 1.0 : 0.0) - 2.0 * (u[i] / n) * (u[j] / n);
  Sym4 s{};
  for (int i = 0; i < 4; ++i)
    for (int j = i; j < 4; ++j) {
      double v = 0.0;
      for (int r = 0; r < 4; ++r) v += Q[i][r] * d[r] * Q[j][r];
      s.a[i][j] = s.a[j][i] = v;
    }
  return s;
}

static void CheckEigen(const Sym4& s, Rng& rng) {
  double M[10], lam[4], y[4];
  s.upper(M);
  TriJacobi4(M, lam, y);
  double fro = 0.0, trace = 0.0;
  for (int i = 0; i < 4; ++i) {
    trace += s.a[i][i];
    for (int j = 0; j < 4; ++j) fro += s.a[i][j] * s.a[i][j];
  }
  fro = std::sqrt(fro);
  double res = 0.0, n2 = 0.0;
  for (int i = 0; i < 4; ++i) {
    double v = -lam[0] * y[i];
    for (int j = 0; j < 4; ++j) v += s.a[i][j] * y[j];
    res += v * v;
    n2 += y[i] * y[i];
  }
  CHECK(std::sqrt(res) <= 64.0 * kEps * fro);
  CHECK(std::fabs(std::sqrt(n2) - 1.0) <= 4.0 * kEps);
  CHECK(lam[0] <= lam[1] && lam[1] <= lam[2] && lam[2] <= lam[3]);
  CHECK(std::fabs((lam[0] + lam[1]) + (lam[2] + lam[3]) - trace) <= 64.0 * kEps * fro);
  // the smallest: M - (l0 - shift) I has a Cholesky factor (shift: a thousand roundings of |M|_F, what the
  // factorization itself may lose), and no Rayleigh quotient is below l0
  if (fro == 0.0) {
    CHECK(lam[0] == 0.0 && lam[3] == 0.0);
    return;
  }
  const double shift = 1000.0 * kEps * fro;
  double L[4][4] = {};
  bool pd = true;
  for (int j = 0; j < 4; ++j) {
    double d = s.a[j][j] - (lam[0] - shift);
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0)) {
      pd = false;
      break;
    }
    L[j][j] = std::sqrt(d);
    for (int i = j + 1; i < 4; ++i) {
      double t = s.a[i][j];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  CHECK(pd);
  for (int trial = 0; trial < 16; ++trial) {
    double x[4], num = 0.0, den = 0.0;
    for (int i = 0; i < 4; ++i) x[i] = trial < 4 ? (i == trial ? 1.0 : 0.0) : rng.sym();
    for (int i = 0; i < 4; ++i) {
      den += x[i] * x[i];
      for (int j = 0; j < 4; ++j) num += x[i] * s.a[i][j] * x[j];
    }
    CHECK(num / den >= lam[0] - 64.0 * kEps * fro);
  }
}

static void JacobiCases() {
  Rng rng{12345};
  const double scales[] = {1.0, 1e-8, 1e8, 3.7e3};
  for (double sc : scales) {
    for (int rep = 0; rep < 200; ++rep) {
      g_case = "jacobi random symmetric";
      Sym4 s{};
      for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j) s.a[i][j] = s.a[j][i] = sc * rng.sym();
      CheckEigen(s, rng);
      for (int rows : {8, 4, 3, 2, 1}) {
        g_case = "jacobi A^T A, rows " + std::to_string(rows);
        std::vector<double> A(4 * (size_t)rows);
        for (double& v : A) v = sc * rng.sym();
        CheckEigen(Gram(A, rows), rng);
      }
      g_case = "jacobi repeated eigenvalues";
      const double specs[][4] = {{1, 1, 2, 2}, {1, 1, 1, 2}, {2, 1, 1, 1}, {1, 1, 1, 1}, {0, 0, 1, 1}, {0, 0, 0, 1},
                                 {-1, -1, 2, 3}, {1e-9, 1e-9, 1, 1}};
      for (const auto& sp : specs) {
        double d[4];
        for (int i = 0; i < 4; ++i) d[i] = sc * sp[i];
        CheckEigen(FromSpectrum(rng, d), rng);
      }
      g_case = "jacobi diagonal";
      Sym4 dg{};
      for (int i = 0; i < 4; ++i) dg.a[i][i] = sc * rng.sym();
      CheckEigen(dg, rng);
    }
  }
  g_case = "jacobi zero";
  CheckEigen(Sym4{}, rng);
  g_case = "jacobi identity";
  Sym4 id{};
  for (int i = 0; i < 4; ++i) id.a[i][i] = 1.0;
  CheckEigen(id, rng);
  g_case = "jacobi non-finite";
  double M[10] = {1, 2, 3, 4, 5, 6, NAN, 8, 9, 10}, lam[4], y[4];
  TriJacobi4(M, lam, y);
  CHECK(TriEigenStatus(lam, y) == SG_TRI_DEGENERATE);
}

static void UndistortCases() {
  const double ks[2][7] = {{-0.1, 0.02, 0.0, 416.0, -416.0, 320.0, 240.0}, {0.0, 0.0, 0.0, 416.0, -416.0, 320.0, 240.0}};
  for (const auto& k : ks) {
    g_case = k[0] != 0.0 ? "undistort k = (-0.1, 0.02, 0)" : "undistort k = 0";
    double worst = 0.0;
    for (int v = 0; v < 480; ++v)
      for (int u = 0; u < 640; ++u) {
        const double pt[2] = {u + 0.25, v + 0.75};
        double ab[2];
        UndistortPixel(k, pt, ab);
        const double r2 = ab[0] * ab[0] + ab[1] * ab[1];
        const double d = 1.0 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]));
        const double e0 = ab[0] * d * k[3] + k[5] - pt[0], e1 = ab[1] * d * k[4] + k[6] - pt[1];
        worst = std::fmax(worst, std::sqrt(e0 * e0 + e1 * e1));
      }
    printf("%s: worst round trip %.3e px\n", g_case.c_str(), worst);
    CHECK(worst <= 1e-9);
    const double centre[2] = {k[5], k[6]};
    double ab[2] = {7, 7};
    UndistortPixel(k, centre, ab);
    CHECK(ab[0] == 0.0 && ab[1] == 0.0);
  }
}

// Identity rotations, pinhole pixels without a cheirality test.
struct Views {
  std::vector<double> q, t, k, pt;
  int n = 0;
  void add(const double* c, const double* P, double du = 0.0, double dv = 0.0) {
    const double K[7] = {0, 0, 0, 416.0, -416.0, 320.0, 240.0};
    const double p[3] = {P[0] - c[0], P[1] - c[1], P[2] - c[2]};
    q.insert(q.end(), {0.0, 0.0, 0.0, 1.0});
    t.insert(t.end(), c, c + 3);
    k.insert(k.end(), K, K + 7);
    pt.push_back(K[3] * p[0] / p[2] + K[5] + du);
    pt.push_back(K[4] * p[1] / p[2] + K[6] + dv);
    ++n;
  }
  sg_triangulate_result run(double min_parallax = 0.0, double max_error_px = 0.0) const {
    sg_triangulate_options o{};
    o.min_parallax = min_parallax;
    o.max_error_px = max_error_px;
    sg_triangulate_result r;
    TriangulatePoint(n, q.data(), t.data(), k.data(), pt.data(), o, &r);
    return r;
  }
};

static bool AllZero(const sg_triangulate_result& r) {
  return r.X[0] == 0.0 && r.X[1] == 0.0 && r.X[2] == 0.0 && r.X[3] == 0.0;
}

static void PointCases() {
  const double c0[3] = {0, 0, 0}, c1[3] = {0, 0, 1000}, c2[3] = {150, 0, 0};
  const double P[3] = {100, 50, 2000}, Pneg[3] = {100, 50, -2000}, Pmid[3] = {30, 20, 500}, Paxis[3] = {0, 0, 3000};
  {
    g_case = "exact two-view point";
    Views v;
    v.add(c0, P);
    v.add(c2, P);
    const sg_triangulate_result r = v.run();
    CHECK(r.status == SG_TRI_OK && r.num_obs == 2);
    CHECK(r.X[3] > 0.0);
    CHECK(std::fabs(std::sqrt(r.X[0] * r.X[0] + r.X[1] * r.X[1] + r.X[2] * r.X[2] + r.X[3] * r.X[3]) - 1.0) <= 4 * kEps);
    for (int j = 0; j < 3; ++j) CHECK(std::fabs(r.X[j] / r.X[3] - P[j]) <= 1e-6);
    CHECK(r.max_error_px <= 1e-9);
    CHECK(std::fabs(r.parallax - std::atan2(150.0 * std::sqrt(50.0 * 50 + 2000.0 * 2000), 100.0 * -50 + 50 * 50 + 2000.0 * 2000)) <= 1e-12);
    CHECK(r.rel_gap > kTriMinRelGap);
    g_case = "gates";
    CHECK(v.run(0.5, 0.0).status == SG_TRI_LOW_PARALLAX);
    CHECK(v.run(0.01, 0.5).status == SG_TRI_OK);
    Views w;
    w.add(c0, P);
    w.add(c2, P, 0.0, 3.0);
    CHECK(w.run(0.0, 0.5).status == SG_TRI_HIGH_ERROR);
    CHECK(w.run(0.5, 0.5).status == SG_TRI_LOW_PARALLAX);   // the first rule that applies
    const sg_triangulate_result g = w.run(0.0, 0.5);
    CHECK(g.max_error_px > 0.5 && g.max_error_px < 3.0 && !AllZero(g));
    CHECK(w.run().status == SG_TRI_OK);
  }
  {
    g_case = "between two cameras that face the same way";
    Views v;
    v.add(c0, Pmid);
    v.add(c1, Pmid);
    const sg_triangulate_result r = v.run();
    CHECK(r.status == SG_TRI_BEHIND && !AllZero(r));
    for (int j = 0; j < 3; ++j) CHECK(std::fabs(r.X[j] / r.X[3] - Pmid[j]) <= 1e-6);
  }
  {
    g_case = "behind both cameras";
    Views v;
    v.add(c0, Pneg);
    v.add(c2, Pneg);
    const sg_triangulate_result r = v.run();
    CHECK(r.status == SG_TRI_BEHIND && r.X[3] > 0.0);
    for (int j = 0; j < 3; ++j) CHECK(std::fabs(r.X[j] / r.X[3] - Pneg[j]) <= 1e-6);
  }
  {
    g_case = "one centre";
    Views v;
    v.add(c0, P);
    v.add(c0, P);
    const sg_triangulate_result r = v.run();
    CHECK(r.status == SG_TRI_NO_BASELINE && AllZero(r) && r.num_obs == 2);
  }
  {
    g_case = "one observation";
    Views v;
    v.add(c0, P);
    const sg_triangulate_result r = v.run();
    CHECK(r.status == SG_TRI_DID_NOT_RUN && AllZero(r) && r.num_obs == 1);
  }
  {
    g_case = "point on the baseline";
    Views v;
    for (int rep = 0; rep < 2; ++rep) {
      v.add(c0, Paxis);
      v.add(c1, Paxis);
    }
    const sg_triangulate_result r = v.run();
    CHECK(r.status == SG_TRI_DEGENERATE && AllZero(r) && r.num_obs == 4);
  }
  {
    g_case = "non-finite pixel";
    Views v;
    v.add(c0, P);
    v.add(c2, P, NAN);
    CHECK(v.run().status == SG_TRI_DEGENERATE);
  }
  {
    g_case = "parallel rays: a point at infinity";
    Views v;
    v.add(c0, Paxis);
    v.add(c2, Paxis);
    v.pt[2] = v.pt[0];   // the second view sees it at the principal point too
    const sg_triangulate_result r = v.run();
    CHECK(r.status == SG_TRI_OK);
    CHECK(std::fabs(r.X[3]) <= 1e-12 && r.X[2] > 0.999);   // (0, 0, 1, 0): in front of the first camera
    CHECK(r.parallax <= 1e-9);
  }
}

int main() {
  JacobiCases();
  UndistortCases();
  PointCases();
  if (g_fail) {
    printf("triangulate_math_check: %d failures\n", g_fail);
    return 1;
  }
  printf("triangulate_math_check OK\n");
  return 0;
}
