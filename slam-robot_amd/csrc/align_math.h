// align_math.h — the per-hypothesis arithmetic of sg_slam_align_points (Sim(3) RANSAC on matched landmarks,
// ba_align.hip), device code that also compiles on the host: k_align_ransac, k_align_select and the CPU check
// (tests/native/align_math_check.cpp) run this one copy.
//
// The similarity Y = s R(q) X + t that best maps the points X onto the points Y in the least-squares sense, by Horn's
// closed form (B. K. P. Horn, "Closed-form solution of absolute orientation using unit quaternions", JOSA A 4, 1987).
// The same function serves a three-record sample and all the inliers of a group:
//   1. centroids xm, ym; centred x' = X - xm, y' = Y - ym; S_ab = sum x'_a y'_b (nine sums), sum |x'|^2, sum |y'|^2
//      (AlignMomentsAdd: always from centred coordinates, never from raw second moments: map coordinates are thousands
//      of units against spreads of hundreds);
//   2. the symmetric 4x4 N in (w, x, y, z) order:
//          Sxx+Syy+Szz   Syz-Szy        Szx-Sxz        Sxy-Syx
//                        Sxx-Syy-Szz    Sxy+Syx        Szx+Sxz
//                                      -Sxx+Syy-Szz    Syz+Szy
//                                                     -Sxx-Syy+Szz
//      q is the unit eigenvector of its largest eigenvalue: TriJacobi4 (triangulate_math.h) on -N, whose smallest
//      eigenpair that is.  l3 >= l2 the two largest eigenvalues of N: gap = (l3 - l2) / l3, which is
//      2 (s2 + s3) / (s1 + s2 + s3) in the singular values of S for a proper match: 0 for collinear points (the
//      rotation about the line is free), of order one for a spread set;
//   3. s = sqrt(sum |y'|^2 / sum |x'|^2), or 1 with fix_scale; t = ym - s R xm;
//   4. no model when a value is not finite, either spread is 0, l3 <= 0, gap <= kAlignMinGap, or s is outside
//      [1 / max_scale, max_scale] (max_scale == 0: no gate).
// q is in Eigen memory [x, y, z, w] with w >= 0.
#ifndef SG_ALIGN_MATH_H_
#define SG_ALIGN_MATH_H_

#include <math.h>

#include "triangulate_math.h"

namespace sg {

// A sample (or an inlier set) whose N matrix has a relative gap at or below this gives no model.
constexpr double kAlignMinGap = 1e-12;
constexpr int kAlignMoments = 11;   // S row-major (S[3 a + b] = sum x'_a y'_b), sum |x'|^2, sum |y'|^2

struct AlignXf {
  double s, q[4], t[3];
};

// A = s R(q), row-major; R is TriRotation's (the standard matrix of a unit quaternion).
SG_HD void AlignMatrix(double s, const double* q, double* A) {
  TriRotation(q, A);
  for (int i = 0; i < 9; ++i) A[i] *= s;
}

// |Y - (A X + t)|^2, the squared residual of one record in b's coordinates.
SG_HD double AlignResidual2(const double* A, const double* t, const double* X, const double* Y) {
  const double d0 = Y[0] - (A[0] * X[0] + A[1] * X[1] + A[2] * X[2] + t[0]);
  const double d1 = Y[1] - (A[3] * X[0] + A[4] * X[1] + A[5] * X[2] + t[1]);
  const double d2 = Y[2] - (A[6] * X[0] + A[7] * X[1] + A[8] * X[2] + t[2]);
  return d0 * d0 + d1 * d1 + d2 * d2;
}

// Step 1: adds one record's centred moments to M.
SG_HD void AlignMomentsAdd(const double* X, const double* Y, const double* xm, const double* ym, double* M) {
  const double x[3] = {X[0] - xm[0], X[1] - xm[1], X[2] - xm[2]};
  const double y[3] = {Y[0] - ym[0], Y[1] - ym[1], Y[2] - ym[2]};
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) M[3 * a + b] += x[a] * y[b];
  M[9] += x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  M[10] += y[0] * y[0] + y[1] * y[1] + y[2] * y[2];
}

// Steps 2-4 from the centroids and the centred moments.  *gap receives the relative gap whenever it is a finite
// number, and 0 otherwise, also when the function returns false.
SG_HD bool AlignFromMoments(const double* xm, const double* ym, const double* M, int fix_scale, double max_scale,
                            AlignXf* out, double* gap) {
  *gap = 0.0;
  const double Sxx = M[0], Sxy = M[1], Sxz = M[2], Syx = M[3], Syy = M[4], Syz = M[5], Szx = M[6], Szy = M[7],
               Szz = M[8];
  // -N, 10 upper entries row-major: 00 01 02 03 11 12 13 22 23 33
  const double negN[10] = {-(Sxx + Syy + Szz), -(Syz - Szy), -(Szx - Sxz), -(Sxy - Syx), -(Sxx - Syy - Szz),
                           -(Sxy + Syx),       -(Szx + Sxz), -(-Sxx + Syy - Szz), -(Syz + Szy), -(-Sxx - Syy + Szz)};
  double lam[4], y[4];
  TriJacobi4(negN, lam, y);
  const double l3 = -lam[0], l2 = -lam[1];
  bool finite = TriFinite(M[9]) && TriFinite(M[10]);
  for (int i = 0; i < 4; ++i) finite = finite && TriFinite(lam[i]) && TriFinite(y[i]);
  if (!finite || !(M[9] > 0.0) || !(M[10] > 0.0) || !(l3 > 0.0)) return false;
  const double g = (l3 - l2) / l3;
  if (!TriFinite(g)) return false;
  *gap = g;
  if (!(g > kAlignMinGap)) return false;
  const double s = fix_scale ? 1.0 : sqrt(M[10] / M[9]);
  if (!TriFinite(s) || !(s > 0.0)) return false;
  if (max_scale != 0.0 && !(s <= max_scale && s * max_scale >= 1.0)) return false;
  const double sg = y[0] < 0.0 ? -1.0 : 1.0;
  out->s = s;
  out->q[0] = sg * y[1];
  out->q[1] = sg * y[2];
  out->q[2] = sg * y[3];
  out->q[3] = sg * y[0];
  double A[9];
  AlignMatrix(s, out->q, A);
  for (int r = 0; r < 3; ++r) {
    out->t[r] = ym[r] - (A[3 * r] * xm[0] + A[3 * r + 1] * xm[1] + A[3 * r + 2] * xm[2]);
    if (!TriFinite(out->t[r])) return false;
  }
  return true;
}

// The whole of steps 1-4 on n records in the order given (six doubles each: X then Y).  The sample of a hypothesis
// (n = 3) on the device, and any record list on the host.
SG_HD bool AlignHorn(const double* rec, int n, int fix_scale, double max_scale, AlignXf* out, double* gap) {
  double xm[3] = {0, 0, 0}, ym[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) {
      xm[c] += rec[6 * i + c];
      ym[c] += rec[6 * i + 3 + c];
    }
  for (int c = 0; c < 3; ++c) {
    xm[c] /= n;
    ym[c] /= n;
  }
  double M[kAlignMoments];
  for (int i = 0; i < kAlignMoments; ++i) M[i] = 0.0;
  for (int i = 0; i < n; ++i) AlignMomentsAdd(rec + 6 * i, rec + 6 * i + 3, xm, ym, M);
  return AlignFromMoments(xm, ym, M, fix_scale, max_scale, out, gap);
}

// The first of sg_align_status' rules that applies to a group that ran and has a model.
SG_HD int AlignStatus(int inliers, double gap, int min_inliers, double min_gap) {
  if (inliers < (min_inliers > 4 ? min_inliers : 4)) return SG_ALIGN_FEW_INLIERS;
  if (gap < min_gap) return SG_ALIGN_DEGENERATE;
  return SG_ALIGN_OK;
}

}  // namespace sg

#endif  // SG_ALIGN_MATH_H_
