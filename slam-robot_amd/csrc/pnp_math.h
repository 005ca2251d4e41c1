// pnp_math.h — the per-hypothesis arithmetic of sg_slam_localize_frames (P3P RANSAC, ba_localize.hip), device code
// that also compiles on the host: k_pose_ransac, k_pose_select and the CPU check (tests/native/pnp_math_check.cpp)
// run this one copy.
//
//   PnpSample        three distinct record indices from a counter-based hash of (seed, frame, hypothesis);
//   PnpEuclidean     homogeneous point -> X.xyz / X.w, refusing |X.w| < kPnpMinW;
//   PnpBearing       pixel -> unit bearing in the camera frame (UndistortPixel, project_math.h);
//   P3pSetup         the sample's three cosines and three squared distances, or "degenerate";
//   P3pQuartic       Grunert's quartic in v = s3 / s1, solved in closed form (Ferrari, real roots only);
//   P3pPose          one root -> depths (three Newton steps on the distance equations) -> rotation by two
//                    orthonormal triads -> the project's pose (q Eigen [x,y,z,w] with q.w >= 0, t the camera centre);
//   PnpScore         one record's MSAC term min(e^2, tau^2) at a pose, with Project's behind-camera rule.
//
// Why Grunert: the elimination is three lines (below), the quartic's coefficients are formed as polynomial
// products, so there is no table of hand-expanded terms to get wrong, and the closed form is only a starting point:
// each root is polished on the three distance equations, which are the problem itself and are well conditioned
// whenever the sample is.  What the polish cannot reach (a root lost to a vanishing denominator, a near-zero leading
// coefficient) costs one hypothesis out of hundreds.
//
// The P3P equations.  Unit bearings f1, f2, f3, Euclidean points P1, P2, P3, depths s_i > 0 with camera points
// Y_i = s_i f_i.  With ca = f2 . f3, cb = f1 . f3, cg = f1 . f2 and a2 = |P2 - P3|^2, b2 = |P1 - P3|^2,
// c2 = |P1 - P2|^2:
//     s2^2 + s3^2 - 2 s2 s3 ca = a2,   s1^2 + s3^2 - 2 s1 s3 cb = b2,   s1^2 + s2^2 - 2 s1 s2 cg = c2.
// Put s2 = u s1, s3 = v s1, divide by the middle equation, K = (a2 - c2) / b2, m = c2 / b2:
//     first - third:   2 u (cg - v ca) = (K - 1) v^2 - 2 K cb v + (K + 1)          u = N(v) / (2 D(v))
//     third:           u^2 - 2 u cg + Q(v) = 0,  Q = 1 - m (1 + v^2 - 2 v cb)
//     together:        N^2 - 4 cg N D + 4 Q D^2 = 0                                  (degree 4 in v)
// and s1 = sqrt(b2 / (1 + v^2 - 2 v cb)).
#ifndef SG_PNP_MATH_H_
#define SG_PNP_MATH_H_

#include <float.h>
#include <stdint.h>

#include "project_math.h"

namespace sg {

// A sample containing a point with |X.w| below this yields no model.  X has unit 4-norm, so |X.w| = 1 / sqrt(1 +
// |P|^2) for the Euclidean P = X.xyz / X.w: the limit is a point 1e9 map units (1000 km at the robot's millimetres)
// from the origin, beyond which P's three coordinates no longer resolve a baseline of metres in fp64.
constexpr double kPnpMinW = 1e-9;
// Two directions count as equal, and three points as collinear, when the squared sine of their angle is below this.
constexpr double kPnpMinSin2 = 1e-20;

SG_HD bool PnpFinite(double x) { return fabs(x) <= DBL_MAX; }   // (false for NaN)

// The integer hash of the sampler: the 32-bit finalizer "lowbias32" (xor-shift 16, * 0x7feb352d, xor-shift 15,
// * 0x846ca68b, xor-shift 16), all arithmetic modulo 2^32.
SG_HD uint32_t PnpMix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// r in [0, 2^32) -> [0, n): the high word of the 64-bit product r * n.
SG_HD uint32_t PnpBelow(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * (uint64_t)n) >> 32); }

// Hypothesis h of map frame f: base = mix(mix(mix(seed) + f) + h), r_j = mix(base ^ (0x9e3779b9 * (j + 1))) for
// j = 0, 1, 2; i0 = below(r_0, n), i1 = below(r_1, n - 1), i2 = below(r_2, n - 2); then i1 skips over i0
// (i1 >= i0: i1 + 1) and i2 over both in ascending order (lo = min(i0, i1), hi = max(i0, i1); i2 >= lo: i2 + 1,
// then i2 >= hi: i2 + 1).  n >= 3.  Nothing is carried from one hypothesis to the next.
SG_HD void PnpSample(uint32_t seed, int32_t f, int32_t h, int32_t n, int32_t* idx) {
  const uint32_t base = PnpMix(PnpMix(PnpMix(seed) + (uint32_t)f) + (uint32_t)h);
  const uint32_t r0 = PnpMix(base ^ 0x9e3779b9u);
  const uint32_t r1 = PnpMix(base ^ (0x9e3779b9u * 2u));
  const uint32_t r2 = PnpMix(base ^ (0x9e3779b9u * 3u));
  const int32_t i0 = (int32_t)PnpBelow(r0, (uint32_t)n);
  int32_t i1 = (int32_t)PnpBelow(r1, (uint32_t)(n - 1));
  int32_t i2 = (int32_t)PnpBelow(r2, (uint32_t)(n - 2));
  if (i1 >= i0) ++i1;
  const int32_t lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
  if (i2 >= lo) ++i2;
  if (i2 >= hi) ++i2;
  idx[0] = i0;
  idx[1] = i1;
  idx[2] = i2;
}

// Pixel -> unit bearing (a, b, 1) / |(a, b, 1)| with (a, b) the undistorted plane coordinates.
SG_HD void PnpBearing(const double* k, const double* pt, double* f) {
  double ab[2];
  UndistortPixel(k, pt, ab);
  const double s = 1.0 / sqrt(ab[0] * ab[0] + ab[1] * ab[1] + 1.0);
  f[0] = ab[0] * s;
  f[1] = ab[1] * s;
  f[2] = s;
}

// Homogeneous X (unit 4-norm) -> Euclidean P = X.xyz / X.w.  False (the sample yields no model) when |X.w| is below
// kPnpMinW or not a number.
SG_HD bool PnpEuclidean(const double* X, double* P) {
  if (!(fabs(X[3]) >= kPnpMinW)) return false;
  const double iw = 1.0 / X[3];
  P[0] = X[0] * iw;
  P[1] = X[1] * iw;
  P[2] = X[2] * iw;
  return true;
}

struct P3pProblem {
  double ca, cb, cg;   // f2 . f3, f1 . f3, f1 . f2
  double a2, b2, c2;   // |P2 - P3|^2, |P1 - P3|^2, |P1 - P2|^2
};

SG_HD double pnp_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
SG_HD void pnp_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
// 1 - cos^2 of the angle between a and b, times |a|^2 |b|^2: |a x b|^2.
SG_HD double pnp_cross2(const double* a, const double* b) {
  double c[3];
  pnp_cross(a, b, c);
  return pnp_dot(c, c);
}

// f[3][3] unit bearings, P[3][3] Euclidean points.  False (no model) when a value is not finite, two bearings are
// equal, or the three points are collinear (two equal points included).
SG_HD bool P3pSetup(const double (*f)[3], const double (*P)[3], P3pProblem* pr) {
  double e1[3], e2[3], e3[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    e1[i] = P[1][i] - P[0][i];
    e2[i] = P[2][i] - P[0][i];
    e3[i] = P[2][i] - P[1][i];
  }
  pr->a2 = pnp_dot(e3, e3);
  pr->b2 = pnp_dot(e2, e2);
  pr->c2 = pnp_dot(e1, e1);
  pr->ca = pnp_dot(f[1], f[2]);
  pr->cb = pnp_dot(f[0], f[2]);
  pr->cg = pnp_dot(f[0], f[1]);
  const double sum = (pr->a2 + pr->b2 + pr->c2) + (pr->ca + pr->cb + pr->cg);
  if (!PnpFinite(sum)) return false;
  if (!(pnp_cross2(e1, e2) > kPnpMinSin2 * (pr->c2 * pr->b2))) return false;
  if (!(pnp_cross2(f[0], f[1]) > kPnpMinSin2) || !(pnp_cross2(f[0], f[2]) > kPnpMinSin2) ||
      !(pnp_cross2(f[1], f[2]) > kPnpMinSin2))
    return false;
  return true;
}

// Largest real root of z^3 + a2 z^2 + a1 z + a0 (trigonometric form with three real roots, Cardano with one), then
// two Newton steps.
SG_HD double pnp_cubic_largest(double a2, double a1, double a0) {
  const double Q = (a2 * a2 - 3.0 * a1) / 9.0;
  const double R = (2.0 * a2 * a2 * a2 - 9.0 * a2 * a1 + 27.0 * a0) / 54.0;
  const double Q3 = Q * Q * Q;
  double z;
  if (R * R < Q3) {
    const double th = acos(R / sqrt(Q3));
    z = -2.0 * sqrt(Q) * cos((th + 6.283185307179586) / 3.0) - a2 / 3.0;
  } else {
    const double A = -copysign(cbrt(fabs(R) + sqrt(R * R - Q3)), R);
    const double B = A != 0.0 ? Q / A : 0.0;
    z = (A + B) - a2 / 3.0;
  }
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double fz = ((z + a2) * z + a1) * z + a0;
    const double dz = (3.0 * z + 2.0 * a2) * z + a1;
    if (dz != 0.0) z -= fz / dz;
  }
  return z;
}

// Real roots of y^2 + B y + C appended to x (shifted by -shift); a discriminant that is negative only by rounding
// counts as a double root.
SG_HD int pnp_quadratic(double B, double C, double shift, double* x, int n) {
  double disc = B * B - 4.0 * C;
  if (!(disc >= -1e-12 * (B * B + fabs(4.0 * C)))) return n;
  if (disc < 0.0) disc = 0.0;
  const double s = sqrt(disc);
  x[n++] = 0.5 * (-B + s) - shift;
  x[n++] = 0.5 * (-B - s) - shift;
  return n;
}

// Real roots of A[0] x^4 + A[1] x^3 + A[2] x^2 + A[3] x + A[4] by Ferrari: depress with x = y - b / 4 to
// y^4 + p y^2 + q y + r, take the largest real root m of the resolvent 8 m^3 + 8 p m^2 + (2 p^2 - 8 r) m - q^2 = 0
// (m >= 0 since the resolvent is -q^2 <= 0 at 0), and split into y^2 -+ sqrt(2m) y + p/2 + m +- q / (2 sqrt(2m)).
// m == 0 (then q == 0) is the biquadratic.  Returns the number of roots written to x (0 .. 4), in this order:
// the first quadratic's larger and smaller root, then the second's.
SG_HD int pnp_quartic(const double* A, double* x) {
  if (!(fabs(A[0]) > 0.0)) return 0;
  const double inv = 1.0 / A[0];
  const double b = A[1] * inv, c = A[2] * inv, d = A[3] * inv, e = A[4] * inv;
  if (!PnpFinite((b + c) + (d + e))) return 0;
  const double b2 = b * b;
  const double p = c - 0.375 * b2;
  const double q = d - 0.5 * b * c + 0.125 * b2 * b;
  const double r = e - 0.25 * b * d + 0.0625 * b2 * c - (3.0 / 256.0) * b2 * b2;
  const double shift = 0.25 * b;
  const double m = pnp_cubic_largest(p, 0.25 * p * p - r, -0.125 * q * q);
  int n = 0;
  if (m > 0.0 && PnpFinite(m)) {
    const double sq = sqrt(2.0 * m);
    const double g = q / (2.0 * sq);
    n = pnp_quadratic(-sq, 0.5 * p + m + g, shift, x, n);
    n = pnp_quadratic(sq, 0.5 * p + m - g, shift, x, n);
  } else if (m == 0.0) {
    // y^4 + p y^2 + r: y^2 = z with z^2 + p z + r = 0
    double z[2];
    const int nz = pnp_quadratic(p, r, 0.0, z, 0);
    for (int i = 0; i < nz; ++i)
      if (z[i] >= 0.0) {
        const double s = sqrt(z[i]);
        x[n++] = s - shift;
        x[n++] = -s - shift;
      }
  }
  return n;
}

// Grunert's quartic in v for the problem pr: returns the number of real roots written to v (0 .. 4), in
// pnp_quartic's order.  The position in this list is the hypothesis' "root index".
SG_HD int P3pQuartic(const P3pProblem& pr, double* v) {
  const double ib2 = 1.0 / pr.b2;
  const double K = (pr.a2 - pr.c2) * ib2, m = pr.c2 * ib2;
  const double n2 = K - 1.0, n1 = -2.0 * K * pr.cb, n0 = K + 1.0;   // N(v)
  const double d1 = -pr.ca, d0 = pr.cg;                             // D(v)
  const double q2 = -m, q1 = 2.0 * m * pr.cb, q0 = 1.0 - m;         // Q(v)
  const double g = 4.0 * pr.cg;
  double A[5];
  A[0] = n2 * n2 + 4.0 * (q2 * d1 * d1);
  A[1] = 2.0 * n2 * n1 - g * (n2 * d1) + 4.0 * (2.0 * q2 * d1 * d0 + q1 * d1 * d1);
  A[2] = (n1 * n1 + 2.0 * n2 * n0) - g * (n2 * d0 + n1 * d1) + 4.0 * (q2 * d0 * d0 + 2.0 * q1 * d1 * d0 + q0 * d1 * d1);
  A[3] = 2.0 * n1 * n0 - g * (n1 * d0 + n0 * d1) + 4.0 * (q1 * d0 * d0 + 2.0 * q0 * d1 * d0);
  A[4] = n0 * n0 - g * (n0 * d0) + 4.0 * (q0 * d0 * d0);
  return pnp_quartic(A, v);
}

// Rotation matrix (row-major, world -> camera) -> Eigen quaternion memory [x, y, z, w], unit, w >= 0 (Shepperd's
// four branches on the largest of the trace and the diagonal).
SG_HD void PnpQuatFromRotation(const double* R, double* q) {
  const double tr = R[0] + R[4] + R[8];
  double x, y, z, w;
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0) * 2.0;
    w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = sqrt(1.0 + R[0] - R[4] - R[8]) * 2.0;
    w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = sqrt(1.0 + R[4] - R[0] - R[8]) * 2.0;
    w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s;
  } else {
    const double s = sqrt(1.0 + R[8] - R[0] - R[4]) * 2.0;
    w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s;
  }
  double inv = 1.0 / sqrt((x * x + y * y) + (z * z + w * w));
  if (w < 0.0) inv = -inv;
  q[0] = x * inv; q[1] = y * inv; q[2] = z * inv; q[3] = w * inv;
}

// Orthonormal triad of the triangle (A, B, C): x along B - A, z along (B - A) x (C - A), y = z x x.  M row-major,
// rows x, y, z.
SG_HD void pnp_triad(const double* A, const double* B, const double* C, double* M) {
  double e1[3], e2[3], n[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    e1[i] = B[i] - A[i];
    e2[i] = C[i] - A[i];
  }
  pnp_cross(e1, e2, n);
  const double i1 = 1.0 / sqrt(pnp_dot(e1, e1)), i3 = 1.0 / sqrt(pnp_dot(n, n));
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    M[i] = e1[i] * i1;
    M[6 + i] = n[i] * i3;
  }
  pnp_cross(M + 6, M, M + 3);
}

// One root v of P3pQuartic -> the pose.  u = N / (2 D) and s1 from the middle equation give the depths; three Newton
// steps on the three distance equations (3x3, Cramer) take them to rounding; the camera points Y_i = s_i f_i and the
// world points then form congruent triangles, whose orthonormal triads give R = Mc^T Mw, and the camera centre is
// t = mean(P) - R^T mean(Y).  False (no pose) unless every depth is positive and every output finite.
SG_HD bool P3pPose(const double (*f)[3], const double (*P)[3], const P3pProblem& pr, double v, double* q, double* t) {
  if (!(v > 0.0)) return false;
  const double ib2 = 1.0 / pr.b2;
  const double K = (pr.a2 - pr.c2) * ib2;
  const double u = ((K - 1.0) * v * v - 2.0 * K * pr.cb * v + (K + 1.0)) / (2.0 * (pr.cg - v * pr.ca));
  const double den = 1.0 + v * v - 2.0 * v * pr.cb;
  if (!(u > 0.0) || !(den > 0.0)) return false;
  double s[3];
  s[0] = sqrt(pr.b2 / den);
  s[1] = u * s[0];
  s[2] = v * s[0];
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const double g0 = s[1] * s[1] + s[2] * s[2] - 2.0 * s[1] * s[2] * pr.ca - pr.a2;
    const double g1 = s[0] * s[0] + s[2] * s[2] - 2.0 * s[0] * s[2] * pr.cb - pr.b2;
    const double g2 = s[0] * s[0] + s[1] * s[1] - 2.0 * s[0] * s[1] * pr.cg - pr.c2;
    // J = [[0, j01, j02], [j10, 0, j12], [j20, j21, 0]]
    const double j01 = 2.0 * (s[1] - s[2] * pr.ca), j02 = 2.0 * (s[2] - s[1] * pr.ca);
    const double j10 = 2.0 * (s[0] - s[2] * pr.cb), j12 = 2.0 * (s[2] - s[0] * pr.cb);
    const double j20 = 2.0 * (s[0] - s[1] * pr.cg), j21 = 2.0 * (s[1] - s[0] * pr.cg);
    const double det = j01 * j12 * j20 + j02 * j10 * j21;
    const double id = 1.0 / det;
    // inverse of J by cofactors, applied to g
    const double d0 = (-j12 * j21) * g0 + (j02 * j21) * g1 + (j01 * j12) * g2;
    const double d1 = (j12 * j20) * g0 + (-j02 * j20) * g1 + (j02 * j10) * g2;
    const double d2 = (j10 * j21) * g0 + (j01 * j20) * g1 + (-j01 * j10) * g2;
    s[0] -= d0 * id;
    s[1] -= d1 * id;
    s[2] -= d2 * id;
  }
  if (!(s[0] > 0.0) || !(s[1] > 0.0) || !(s[2] > 0.0)) return false;
  double Y[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) Y[i][c] = s[i] * f[i][c];
  double Mc[9], Mw[9], R[9];
  pnp_triad(Y[0], Y[1], Y[2], Mc);
  pnp_triad(P[0], P[1], P[2], Mw);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = Mc[i] * Mw[j] + Mc[3 + i] * Mw[3 + j] + Mc[6 + i] * Mw[6 + j];
  PnpQuatFromRotation(R, q);
  double ym[3], pm[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ym[c] = (Y[0][c] + Y[1][c] + Y[2][c]) * (1.0 / 3.0);
    pm[c] = (P[0][c] + P[1][c] + P[2][c]) * (1.0 / 3.0);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) t[c] = pm[c] - (R[c] * ym[0] + R[3 + c] * ym[1] + R[6 + c] * ym[2]);
  const double sum = ((q[0] + q[1]) + (q[2] + q[3])) + (t[0] + t[1] + t[2]);
  return PnpFinite(sum);
}

// One record's MSAC term at the pose (q, t): min(e^2, tau2) with e the pixel error, tau2 when Project refuses the
// point (project.h:27) or the error is not a number.  *inlier = (e^2 <= tau2).
SG_HD double PnpScore(const double* q, const double* t, const double* k, const double* X, const double* pt, double tau2,
                      int* inlier) {
  double uv[2];
  *inlier = 0;
  if (!Project(q, t, k, X, uv)) return tau2;
  const double dx = uv[0] - pt[0], dy = uv[1] - pt[1];
  const double e2 = dx * dx + dy * dy;
  if (!(e2 <= tau2)) return tau2;
  *inlier = 1;
  return e2;
}

}  // namespace sg

#endif  // SG_PNP_MATH_H_
