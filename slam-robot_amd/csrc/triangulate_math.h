// triangulate_math.h — the per-point arithmetic of sg_slam_triangulate_points (linear multi-view triangulation,
// ba_triangulate.hip), device code that also compiles on the host: k_point_triangulate and the CPU check
// (tests/native/triangulate_math_check.cpp) run this one copy.
//
// A point's location from its observations alone, by the homogeneous direct linear transform:
//   1. every observed pixel is undistorted to plane coordinates (a, b) (UndistortPixel, project_math.h);
//   2. the world is shifted and scaled to a local frame, origin c0 = the first record's camera centre and unit
//      L = the rms distance of the records' centres from c0: world units are millimetres and locations are
//      thousands, so the raw 4-column system mixes columns that differ by 1e3 .. 1e4 in scale (1e6 .. 1e8 in
//      M = A^T A); in the local frame the centres are of order one.  L^2 == 0: every ray leaves from one centre;
//   3. each record gives the two rows [n, -n . c_i] with n = a r3 - r1 and n = b r3 - r2 (r1, r2, r3 the rows of
//      the rotation of CameraPoint's _transformVector, c_i = (t_i - c0) / L): p.x - a p.z = 0 and p.y - b p.z = 0
//      for p = R_i (X.xyz - t_i X.w), rewritten in the local frame.  M = sum row^T row, 10 upper entries;
//   4. y = the unit eigenvector of M's smallest eigenvalue, by cyclic Jacobi rotations; the four eigenvalues
//      l0 <= l1 <= l2 <= l3 are kept: l1 - l0 <= kTriMinRelGap l3 means the direction is not determined;
//   5. X = (L y.xyz + c0 y.w, y.w), the sign chosen with X.w >= 0 (X.w == 0: the sign that puts the point in front
//      of the first record's camera), scaled to unit 4-norm as Frame::Unproject leaves it (localmap.cpp:35).  The
//      reference's behind-camera test p.z < 0.001 X.w (project.h:27) by itself accepts a point behind every camera
//      when W < 0 (p.z and W are then both negative); with W >= 0 fixed first the test is the physical one;
//   6. one more sweep at X: the records Project rejects (behind), the largest reprojection error and the largest
//      angle at the point between the ray to a record's centre and the ray to the first record's
//      (atan2(|d_i x d_0|, d_i . d_0) with d_i = X.xyz - t_i X.w: valid as W -> 0, the same for X and -X);
//   7. the status: the first of the rules of TriStatus that applies.
#ifndef SG_TRIANGULATE_MATH_H_
#define SG_TRIANGULATE_MATH_H_

#include <math.h>

#include "points_plan.h"
#include "project_math.h"

namespace sg {

// Upper bound on Jacobi sweeps (6 rotations each).  A 4x4 is at rounding level after 4 to 6; a sweep that finds
// nothing left to rotate ends the loop.
constexpr int kTriMaxSweeps = 12;

// Rows r1, r2, r3 of the rotation CameraPoint applies: p = R v, R = I + 2 w [u]x + 2 [u]x^2 (exact for any |q|).
SG_HD void TriRotation(const double* q, double* R) {
  const double ux = q[0], uy = q[1], uz = q[2], w = q[3];
  R[0] = 1.0 - 2.0 * (uy * uy + uz * uz);
  R[1] = 2.0 * (ux * uy - w * uz);
  R[2] = 2.0 * (ux * uz + w * uy);
  R[3] = 2.0 * (ux * uy + w * uz);
  R[4] = 1.0 - 2.0 * (ux * ux + uz * uz);
  R[5] = 2.0 * (uy * uz - w * ux);
  R[6] = 2.0 * (ux * uz - w * uy);
  R[7] = 2.0 * (uy * uz + w * ux);
  R[8] = 1.0 - 2.0 * (ux * ux + uy * uy);
}

// |t - c0|^2 (step 2)
SG_HD double TriCentreDist2(const double* t, const double* c0) {
  const double d0 = t[0] - c0[0], d1 = t[1] - c0[1], d2 = t[2] - c0[2];
  return d0 * d0 + d1 * d1 + d2 * d2;
}

// Step 3: adds one record's two rows to M (10 upper entries of the symmetric 4x4, row-major: 00 01 02 03 11 12 13
// 22 23 33).  inv_l = 1 / L.
SG_HD void TriAddRows(const double* q, const double* t, const double* k, const double* pt, const double* c0,
                      double inv_l, double* M) {
  double R[9], ab[2];
  TriRotation(q, R);
  UndistortPixel(k, pt, ab);
  const double c[3] = {(t[0] - c0[0]) * inv_l, (t[1] - c0[1]) * inv_l, (t[2] - c0[2]) * inv_l};
  for (int h = 0; h < 2; ++h) {
    double row[4];
    for (int j = 0; j < 3; ++j) row[j] = ab[h] * R[6 + j] - R[3 * h + j];
    row[3] = -(row[0] * c[0] + row[1] * c[1] + row[2] * c[2]);
    int e = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = i; j < 4; ++j) M[e++] += row[i] * row[j];
  }
}

// One Jacobi rotation in the (P, Q) plane of the symmetric A (full storage), accumulated into V's columns.  An
// entry that no longer changes either diagonal neighbour when added a hundredfold is set to zero instead (the
// test of the classical cyclic method: below it a rotation moves nothing but rounding).
template <int P, int Q>
SG_HD void TriRotate(double (*A)[4], double (*V)[4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double g = 100.0 * fabs(apq);
  if (fabs(A[P][P]) + g == fabs(A[P][P]) && fabs(A[Q][Q]) + g == fabs(A[Q][Q])) {
    A[P][Q] = A[Q][P] = 0.0;
    return;
  }
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  // the smaller root of t^2 + 2 theta t - 1 = 0 (theta^2 overflowing gives t = 0: nothing to rotate)
  const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
  const double tau = s / (1.0 + c);
  A[P][P] -= tt * apq;
  A[Q][Q] += tt * apq;
  A[P][Q] = A[Q][P] = 0.0;
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const double arp = A[r][P], arq = A[r][Q];
      A[r][P] = A[P][r] = arp - s * (arq + tau * arp);
      A[r][Q] = A[Q][r] = arq + s * (arp - tau * arq);
    }
    const double vrp = V[r][P], vrq = V[r][Q];
    V[r][P] = vrp - s * (vrq + tau * vrp);
    V[r][Q] = vrq + s * (vrp - tau * vrq);
  }
}

// Orders eigenpairs I and J (I < J) by eigenvalue.
template <int I, int J>
SG_HD void TriOrder(double* lam, double (*V)[4]) {
  if (lam[J] < lam[I]) {
    const double l = lam[I];
    lam[I] = lam[J];
    lam[J] = l;
    for (int r = 0; r < 4; ++r) {
      const double v = V[r][I];
      V[r][I] = V[r][J];
      V[r][J] = v;
    }
  }
}

// Step 4: the eigenvalues of the symmetric 4x4 M (10 upper entries) in ascending order and the unit eigenvector of
// the smallest.  Non-finite input gives non-finite output after kTriMaxSweeps sweeps.
SG_HD void TriJacobi4(const double* M, double* lam, double* y) {
  double A[4][4], V[4][4];
  {
    int e = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = i; j < 4; ++j) {
        A[i][j] = A[j][i] = M[e++];
        V[i][j] = V[j][i] = i == j ? 1.0 : 0.0;
      }
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int sweep = 0; sweep < kTriMaxSweeps; ++sweep) {
    const double off = (fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[0][3])) + (fabs(A[1][2]) + fabs(A[1][3]) + fabs(A[2][3]));
    if (off == 0.0) break;
    TriRotate<0, 1>(A, V);
    TriRotate<0, 2>(A, V);
    TriRotate<0, 3>(A, V);
    TriRotate<1, 2>(A, V);
    TriRotate<1, 3>(A, V);
    TriRotate<2, 3>(A, V);
  }
  for (int i = 0; i < 4; ++i) lam[i] = A[i][i];
  TriOrder<0, 1>(lam, V);
  TriOrder<2, 3>(lam, V);
  TriOrder<0, 2>(lam, V);
  TriOrder<1, 3>(lam, V);
  TriOrder<1, 2>(lam, V);
  // V is orthogonal up to rounding; the column is renormalized so that |y| = 1 to the last bit or two
  const double n = sqrt((V[0][0] * V[0][0] + V[1][0] * V[1][0]) + (V[2][0] * V[2][0] + V[3][0] * V[3][0]));
  for (int r = 0; r < 4; ++r) y[r] = V[r][0] / n;
}

// (l1 - l0) / l3, 0 for the zero matrix
SG_HD double TriRelGap(const double* lam) { return lam[3] > 0.0 ? (lam[1] - lam[0]) / lam[3] : 0.0; }

// Step 5.  q0, t0: the pose of the point's first record.
SG_HD void TriToWorld(const double* y, const double* c0, double l, const double* q0, const double* t0, double* X) {
  for (int j = 0; j < 3; ++j) X[j] = l * y[j] + c0[j] * y[3];
  X[3] = y[3];
  bool flip = X[3] < 0.0;
  if (X[3] == 0.0) {
    double v[3], p[3];
    CameraPoint(q0, t0, X, v, p);
    flip = p[2] < 0.0;
  }
  const double n = sqrt((X[0] * X[0] + X[1] * X[1]) + (X[2] * X[2] + X[3] * X[3]));
  const double s = (flip ? -1.0 : 1.0) / n;
  for (int j = 0; j < 4; ++j) X[j] *= s;
}

// Step 6, one record: counts it in *behind if Project rejects it (it then has no error), otherwise raises *err to
// its reprojection error; raises *par to the angle at X between this record's centre and the first record's (t0).
SG_HD void TriQuality(const double* q, const double* t, const double* k, const double* pt, const double* t0,
                      const double* X, double* behind, double* err, double* par) {
  double uv[2];
  if (!Project(q, t, k, X, uv)) {
    *behind += 1.0;
  } else {
    const double e0 = uv[0] - pt[0], e1 = uv[1] - pt[1];
    *err = fmax(*err, sqrt(e0 * e0 + e1 * e1));
  }
  const double d[3] = {X[0] - t[0] * X[3], X[1] - t[1] * X[3], X[2] - t[2] * X[3]};
  const double d0[3] = {X[0] - t0[0] * X[3], X[1] - t0[1] * X[3], X[2] - t0[2] * X[3]};
  const double c0 = d[1] * d0[2] - d[2] * d0[1], c1 = d[2] * d0[0] - d[0] * d0[2], c2 = d[0] * d0[1] - d[1] * d0[0];
  *par = fmax(*par, atan2(sqrt(c0 * c0 + c1 * c1 + c2 * c2), d[0] * d0[0] + d[1] * d0[1] + d[2] * d0[2]));
}

SG_HD bool TriFinite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN too

// Step 7, after the eigen-solve: SG_TRI_DEGENERATE or SG_TRI_OK (X may be formed).
SG_HD int TriEigenStatus(const double* lam, const double* y) {
  bool finite = true;
  for (int i = 0; i < 4; ++i) finite = finite && TriFinite(lam[i]) && TriFinite(y[i]);
  if (!finite || !(lam[1] - lam[0] > kTriMinRelGap * lam[3])) return SG_TRI_DEGENERATE;
  return SG_TRI_OK;
}

// Step 7, after the quality sweep.  A gate of 0 is off.
SG_HD int TriGateStatus(const double* X, double behind, double err, double par, double min_parallax,
                        double max_error_px) {
  bool finite = TriFinite(err) && TriFinite(par);
  for (int i = 0; i < 4; ++i) finite = finite && TriFinite(X[i]);
  if (!finite) return SG_TRI_DEGENERATE;
  if (behind > 0.0) return SG_TRI_BEHIND;
  if (min_parallax != 0.0 && par < min_parallax) return SG_TRI_LOW_PARALLAX;
  if (max_error_px != 0.0 && err > max_error_px) return SG_TRI_HIGH_ERROR;
  return SG_TRI_OK;
}

// The whole of steps 1-7 for one point on the host, records in the order given (the device sums a point's records
// in its 8-lane order instead; everything else is the code above).  q[4 n], t[3 n], k[7 n], pt[2 n]: the pose,
// intrinsics and pixel of each of the point's n enabled observations.
inline void TriangulatePoint(int n, const double* q, const double* t, const double* k, const double* pt,
                             const sg_triangulate_options& o, sg_triangulate_result* r) {
  *r = sg_triangulate_result{};
  r->num_obs = n;
  r->status = SG_TRI_DID_NOT_RUN;
  if (n < kPointMinObs) return;
  const double* c0 = t;
  double l2 = 0.0;
  for (int i = 0; i < n; ++i) l2 += TriCentreDist2(t + 3 * i, c0);
  l2 /= n;
  r->status = SG_TRI_NO_BASELINE;
  if (l2 == 0.0) return;
  const double l = sqrt(l2), inv_l = 1.0 / l;
  double M[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) TriAddRows(q + 4 * i, t + 3 * i, k + 7 * i, pt + 2 * i, c0, inv_l, M);
  double lam[4], y[4];
  TriJacobi4(M, lam, y);
  r->status = TriEigenStatus(lam, y);
  if (r->status != SG_TRI_OK) return;
  r->rel_gap = TriRelGap(lam);
  double X[4], behind = 0.0, err = 0.0, par = 0.0;
  TriToWorld(y, c0, l, q, t, X);
  for (int i = 0; i < n; ++i) TriQuality(q + 4 * i, t + 3 * i, k + 7 * i, pt + 2 * i, t, X, &behind, &err, &par);
  r->status = TriGateStatus(X, behind, err, par, o.min_parallax, o.max_error_px);
  if (r->status == SG_TRI_DEGENERATE) return;
  r->parallax = par;
  r->max_error_px = err;
  for (int j = 0; j < 4; ++j) r->X[j] = X[j];
}

}  // namespace sg

#endif  // SG_TRIANGULATE_MATH_H_
