// relpose_math.h — the per-hypothesis arithmetic of a two-view relative pose by 8-point RANSAC ("where is frame b
// relative to frame a, from the pixels they share alone"), device code that also compiles on the host: the CPU check
// (tests/native/relpose_math_check.cpp), k_relpose_ransac and k_relpose_select (ba_relpose.hip) run this one copy.
//
//   RelSample             eight distinct record indices from a counter-based hash of (seed, pair key, hypothesis):
//                         PnpSample's three-index scheme (pnp_math.h) extended, PnpMix and PnpBelow as they are;
//   RelNormFrom           Hartley's normalisation of one side: centroid to the origin, rms distance to sqrt 2;
//   RelMomentsAdd         one record's epipolar row (x_b' (x) x_a', nine entries) added into the packed upper triangle
//                         of the symmetric 9x9 moment matrix;
//   EssentialFromMoments  moment matrix -> the unit eigenvector of its smallest eigenvalue -> de-normalised 3x3 ->
//                         projected to singular values (1, 1, 0).  One function for the minimal sample and for a
//                         re-estimate over all inliers;
//   RelSampson            one record's squared Sampson distance in ideal pixels;
//   RelDecompose          E -> the two rotations and the translation direction, det +1;
//   RelDepths             the two depths of a record by the 2x2 least squares of its bearings;
//   RelVote / RelStatus   the decomposition with the most in-front inliers (ties to the earlier); the status rules;
//   RelPoseOut            (R, t) of p_b = R p_a + t -> the map's convention: q_rel (Eigen memory, unit, w >= 0) and
//                         unit t_rel with p_b = q_rel (p_a - t_rel).
// E is row-major with x_b^T E x_a = 0 on plane coordinates (UndistortPixel's output with a third coordinate of 1).
//
// The eigenvector.  M is symmetric positive semi-definite.  A = M + sigma I with sigma = 2^-40 tr(M) is factored as
// L D L^T without pivoting (A is positive definite, so this is Cholesky's stability without the square roots), and
// x <- A^-1 x / |A^-1 x| is repeated from a fixed start until two iterates agree to 1e-15 in every entry, 40 rounds at
// the most; a sample that has not got there gives no model (the convergence factor is (l0 + sigma) / (l1 + sigma):
// 1e-7 and less on a minimal sample, where l0 = 0 to rounding, 5e-3 to 1.3e-2 on the noisy inliers of the tests, so 40
// rounds reach 1e-15 for any factor below 0.42).  Every index below is a compile-time constant after unrolling, so
// the 45 entries stay in registers on the device; a cyclic Jacobi would carry the 81 entries of the eigenvectors as
// well.  The eigenvalues come from iterations too: l0 + sigma = 1 / (x . A^-1 x); l1 + sigma the same for a second
// vector kept orthogonal to x, repeated until it moves by less than 1e-10 relative (40 rounds at the most; a Rayleigh
// quotient of A^-1 on x's complement, so it is never below the true value); l8 the Rayleigh quotient of M after 16
// power iterations from a fixed start (never above the true value, and within a few percent of it after 16 rounds
// since tr(M) <= 9 l8).  A sample gives no model when a value is not finite, a pivot is not positive, x has not
// converged, or (l1 - l0) / l8 <= kRelMinGap.
#ifndef SG_RELPOSE_MATH_H_
#define SG_RELPOSE_MATH_H_

#include <float.h>
#include <stdint.h>

#include "pnp_math.h"
#include "project_math.h"
#include "slamgpu.h"

namespace sg {

constexpr int kRelSample = 8;
constexpr double kRelMinGap = 1e-12;

// Hypothesis h of the pair with key a * 65536 + b: base = mix(mix(mix(seed) + key) + h), r_j = mix(base ^
// (0x9e3779b9 * (j + 1))), i_j = below(r_j, n - j) for j = 0 .. 7; each i_j is then stepped over the earlier indices
// taken in ascending order (i_j >= p: i_j + 1).  n >= 8.  idx is in draw order.  Nothing is carried between hypotheses.
SG_HD void RelSample(uint32_t seed, uint32_t key, int32_t h, int32_t n, int32_t* idx) {
  const uint32_t base = PnpMix(PnpMix(PnpMix(seed) + key) + (uint32_t)h);
  int32_t sorted[kRelSample];
#pragma unroll
  for (int j = 0; j < kRelSample; ++j) {
    const uint32_t r = PnpMix(base ^ (0x9e3779b9u * (uint32_t)(j + 1)));
    int32_t v = (int32_t)PnpBelow(r, (uint32_t)(n - j));
#pragma unroll
    for (int p = 0; p < j; ++p)
      if (v >= sorted[p]) ++v;
    idx[j] = v;
    // insert into the ascending list: carry the larger value upwards
    int32_t carry = v;
#pragma unroll
    for (int p = 0; p < j; ++p) {
      const int32_t s = sorted[p];
      const bool gt = s > carry;
      sorted[p] = gt ? carry : s;
      carry = gt ? s : carry;
    }
    sorted[j] = carry;
  }
}

// Hartley's normalisation of one side from the sums over its points: st = {count, sum x, sum y, sum (x^2 + y^2)}.
// nrm = {cx, cy, s}: x' = s (x - cx), y' = s (y - cy), with the rms distance from the centroid sqrt 2.  False when
// the points coincide or a value is not finite.
SG_HD bool RelNormFrom(const double* st, double* nrm) {
  const double inv = 1.0 / st[0];
  const double cx = st[1] * inv, cy = st[2] * inv;
  const double var = st[3] * inv - (cx * cx + cy * cy);   // mean squared distance from the centroid
  nrm[0] = cx;
  nrm[1] = cy;
  nrm[2] = sqrt(2.0 / var);
  return var > 0.0 && PnpFinite(nrm[2]) && PnpFinite(cx + cy);
}

// Packed upper triangle of the 9x9: entry (i, j), i <= j, at i * (19 - i) / 2 + (j - i).
constexpr int kRelMoments = 45;
SG_HD constexpr int rel_u9(int i, int j) { return i * (19 - i) / 2 + (j - i); }

// The record's row x_b' (x) x_a' = (xb xa, xb ya, xb, yb xa, yb ya, yb, xa, ya, 1) in normalised coordinates.
SG_HD void RelRow(const double* na, const double* nb, const double* xa, const double* xb, double* row) {
  const double ax = na[2] * (xa[0] - na[0]), ay = na[2] * (xa[1] - na[1]);
  const double bx = nb[2] * (xb[0] - nb[0]), by = nb[2] * (xb[1] - nb[1]);
  row[0] = bx * ax; row[1] = bx * ay; row[2] = bx;
  row[3] = by * ax; row[4] = by * ay; row[5] = by;
  row[6] = ax;      row[7] = ay;      row[8] = 1.0;
}

SG_HD void RelMomentsAdd(const double* row, double* M) {
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int j = i; j < 9; ++j) M[rel_u9(i, j)] += row[i] * row[j];
}

// x <- A^-1 x with A = L D L^T held in M's packed triangle: unit L^T above the diagonal, D on it.
SG_HD void rel_ldl_solve(const double* A, double* x) {
#pragma unroll
  for (int i = 1; i < 9; ++i)   // L y = x
#pragma unroll
    for (int k = 0; k < i; ++k) x[i] -= A[rel_u9(k, i)] * x[k];
#pragma unroll
  for (int i = 0; i < 9; ++i) x[i] /= A[rel_u9(i, i)];
#pragma unroll
  for (int i = 7; i >= 0; --i)   // L^T z = y
#pragma unroll
    for (int k = i + 1; k < 9; ++k) x[i] -= A[rel_u9(i, k)] * x[k];
}

// y = M x with M's packed upper triangle.
SG_HD void rel_symv(const double* M, const double* x, double* y) {
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) s += M[i <= j ? rel_u9(i, j) : rel_u9(j, i)] * x[j];
    y[i] = s;
  }
}

SG_HD double rel_dot9(const double* a, const double* b) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) s += a[i] * b[i];
  return s;
}

// Symmetric 3x3 (S row-major, both halves filled) -> eigenvectors in V's columns by cyclic Jacobi, eight sweeps,
// eigenvalues left on S's diagonal; then sorted descending.  Used on E^T E.
SG_HD void rel_jacobi3(double (*S)[3], double (*V)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 8; ++sweep) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double apq = S[p][q];
        if (apq == 0.0) continue;
        const double theta = (S[q][q] - S[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // columns p, q
          const double skp = S[k][p], skq = S[k][q];
          S[k][p] = c * skp - s * skq;
          S[k][q] = s * skp + c * skq;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {   // rows p, q
          const double spk = S[p][k], sqk = S[q][k];
          S[p][k] = c * spk - s * sqk;
          S[q][k] = s * spk + c * sqk;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  // descending by eigenvalue: three compare-exchanges on (0,1), (1,2), (0,1)
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
    const int a = pass == 1 ? 1 : 0, b = a + 1;
    if (S[a][a] < S[b][b]) {
      const double l = S[a][a];
      S[a][a] = S[b][b];
      S[b][b] = l;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double v = V[k][a];
        V[k][a] = V[k][b];
        V[k][b] = v;
      }
    }
  }
}

// G (3x3 row-major) -> its two leading singular pairs completed to rotations: U and V (columns u1 u2 u3, v1 v2 v3,
// u3 = u1 x u2, v3 = v1 x v2, so det U = det V = +1) with G ~ s1 u1 v1^T + s2 u2 v2^T.  V from the Jacobi of G^T G,
// u_i = G v_i normalised, u2 made orthogonal to u1.  False when the second singular value vanishes or a value is not
// finite.
SG_HD bool RelSvd2(const double* G, double (*U)[3], double (*V)[3]) {
  double S[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) S[i][j] = G[i] * G[j] + G[3 + i] * G[3 + j] + G[6 + i] * G[6 + j];
  rel_jacobi3(S, V);
  double u1[3], u2[3], v1[3], v2[3], v3[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    v1[i] = V[i][0];
    v2[i] = V[i][1];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u1[i] = pnp_dot(G + 3 * i, v1);
    u2[i] = pnp_dot(G + 3 * i, v2);
  }
  const double n1 = sqrt(pnp_dot(u1, u1));
#pragma unroll
  for (int i = 0; i < 3; ++i) u1[i] /= n1;
  const double d = pnp_dot(u1, u2);
#pragma unroll
  for (int i = 0; i < 3; ++i) u2[i] -= d * u1[i];
  const double n2 = sqrt(pnp_dot(u2, u2));
  if (!(n2 > 1e-150) || !PnpFinite(n1 + n2) || !(n1 > 0.0)) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i) u2[i] /= n2;
  double u3[3];
  pnp_cross(u1, u2, u3);
  pnp_cross(v1, v2, v3);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    U[i][0] = u1[i]; U[i][1] = u2[i]; U[i][2] = u3[i];
    V[i][2] = v3[i];
  }
  return true;
}

// The nearest matrix to G with singular values (1, 1, 0): u1 v1^T + u2 v2^T, Frobenius norm sqrt 2.
SG_HD bool RelProjectEssential(const double* G, double* E) {
  double U[3][3], V[3][3];
  if (!RelSvd2(G, U, V)) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) E[3 * i + j] = U[i][0] * V[j][0] + U[i][1] * V[j][1];
  return true;
}

// The moment matrix M (packed upper triangle, overwritten) of rows formed with the normalisations na, nb -> E.
// *gap (may be null) receives (l1 - l0) / l8.  False: no model (see the head of the file).
SG_HD bool EssentialFromMoments(double* M, const double* na, const double* nb, double* E, double* gap) {
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) tr += M[rel_u9(i, i)];
  if (!PnpFinite(tr) || !(tr > 0.0)) return false;
  double l8 = 0.0;
  {
    double p[9] = {0.33, 0.31, 0.35, 0.32, 0.36, 0.34, 0.30, 0.37, 0.29}, w[9];
#pragma unroll 1
    for (int it = 0; it < 16; ++it) {
      rel_symv(M, p, w);
      l8 = rel_dot9(p, w) / rel_dot9(p, p);
      const double inv = 1.0 / sqrt(rel_dot9(w, w));
#pragma unroll
      for (int i = 0; i < 9; ++i) p[i] = w[i] * inv;
    }
  }
  if (!PnpFinite(l8) || !(l8 > 0.0)) return false;
  const double sigma = tr * (1.0 / 1099511627776.0);   // 2^-40
#pragma unroll
  for (int i = 0; i < 9; ++i) M[rel_u9(i, i)] += sigma;
  // L D L^T in place, column by column: after step k, row k above the diagonal holds L^T's row k
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double d = M[rel_u9(k, k)];
    ok = ok && d > 0.0;
    const double id = 1.0 / d;
#pragma unroll
    for (int i = k + 1; i < 9; ++i) {
      const double l = M[rel_u9(k, i)] * id;
#pragma unroll
      for (int j = i; j < 9; ++j) M[rel_u9(i, j)] -= l * M[rel_u9(k, j)];
      M[rel_u9(k, i)] = l;
    }
  }
  if (!ok) return false;
  double x[9] = {0.29, -0.21, 0.18, 0.27, -0.33, 0.24, -0.15, 0.36, 0.09};
  double mu0 = 0.0;
  bool converged = false;
  for (int it = 0; it < 40; ++it) {
    double z[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) z[i] = x[i];
    rel_ldl_solve(M, z);
    const double xz = rel_dot9(x, z), xx = rel_dot9(x, x);
    mu0 = xx / xz;   // l0 + sigma once converged
    const double inv = 1.0 / sqrt(rel_dot9(z, z));
    double diff = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const double v = z[i] * inv;
      diff = fmax(diff, fabs(v - x[i]));
      x[i] = v;
    }
    if (diff <= 1e-15) {
      converged = true;
      break;
    }
    if (!(diff > 1e-15)) break;   // (a NaN)
  }
  if (!converged) return false;
  double y[9] = {0.31, 0.22, -0.17, -0.26, 0.12, 0.35, 0.28, -0.14, -0.23};
  double mu1 = 0.0;
#pragma unroll 1
  for (int it = 0; it < 40; ++it) {
    const double xy = rel_dot9(x, y);
#pragma unroll
    for (int i = 0; i < 9; ++i) y[i] -= xy * x[i];
    const double inv = 1.0 / sqrt(rel_dot9(y, y));
    double z[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      y[i] *= inv;
      z[i] = y[i];
    }
    rel_ldl_solve(M, z);
    const double xz = rel_dot9(x, z);
#pragma unroll
    for (int i = 0; i < 9; ++i) z[i] -= xz * x[i];
    const double prev = mu1;
    mu1 = 1.0 / rel_dot9(y, z);   // l1 + sigma, from above
#pragma unroll
    for (int i = 0; i < 9; ++i) y[i] = z[i];
    if (fabs(mu1 - prev) <= 1e-10 * mu1) break;
  }
  const double g = (mu1 - mu0) / l8;
  if (gap) *gap = g;
  if (!PnpFinite(g) || !(g > kRelMinGap)) return false;
  // de-normalise: E = Tb^T E' Ta with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
  double P[9], G[9];
  const double sa = na[2], sb = nb[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) {   // P = E' Ta
    P[3 * r + 0] = x[3 * r + 0] * sa;
    P[3 * r + 1] = x[3 * r + 1] * sa;
    P[3 * r + 2] = x[3 * r + 2] - sa * (x[3 * r + 0] * na[0] + x[3 * r + 1] * na[1]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {   // G = Tb^T P
    G[c] = sb * P[c];
    G[3 + c] = sb * P[3 + c];
    G[6 + c] = P[6 + c] - sb * (P[c] * nb[0] + P[3 + c] * nb[1]);
  }
  if (!RelProjectEssential(G, E)) return false;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) sum += E[i];
  return PnpFinite(sum);
}

// The sample's E: eight records' plane coordinates xa[8][2], xb[8][2].
SG_HD bool RelEightPoint(const double (*xa)[2], const double (*xb)[2], double* E, double* gap) {
  double sa[4] = {8.0, 0.0, 0.0, 0.0}, sb[4] = {8.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sa[1] += xa[i][0]; sa[2] += xa[i][1]; sa[3] += xa[i][0] * xa[i][0] + xa[i][1] * xa[i][1];
    sb[1] += xb[i][0]; sb[2] += xb[i][1]; sb[3] += xb[i][0] * xb[i][0] + xb[i][1] * xb[i][1];
  }
  double na[3], nb[3];
  if (!RelNormFrom(sa, na) || !RelNormFrom(sb, nb)) return false;
  double M[kRelMoments];
#pragma unroll
  for (int i = 0; i < kRelMoments; ++i) M[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    double row[9];
    RelRow(na, nb, xa[i], xb[i], row);
    RelMomentsAdd(row, M);
  }
  return EssentialFromMoments(M, na, nb, E, gap);
}

// Squared Sampson distance of one record in ideal pixels: F = K_b^-T E K_a^-1 on (fx x + cx, fy y + cy), which in
// plane coordinates is (x_b^T E x_a)^2 / ((l_1 / fx_b)^2 + (l_2 / fy_b)^2 + (m_1 / fx_a)^2 + (m_2 / fy_a)^2) with
// l = E x_a and m = E^T x_b.  ifa = {1 / fx_a, 1 / fy_a}, ifb likewise.  May be NaN or infinite; the caller
// truncates.
SG_HD double RelSampson(const double* E, const double* xa, const double* xb, const double* ifa, const double* ifb) {
  const double l0 = E[0] * xa[0] + E[1] * xa[1] + E[2];
  const double l1 = E[3] * xa[0] + E[4] * xa[1] + E[5];
  const double l2 = E[6] * xa[0] + E[7] * xa[1] + E[8];
  const double m0 = E[0] * xb[0] + E[3] * xb[1] + E[6];
  const double m1 = E[1] * xb[0] + E[4] * xb[1] + E[7];
  const double r = xb[0] * l0 + xb[1] * l1 + l2;
  const double a0 = l0 * ifb[0], a1 = l1 * ifb[1], b0 = m0 * ifa[0], b1 = m1 * ifa[1];
  return (r * r) / ((a0 * a0 + a1 * a1) + (b0 * b0 + b1 * b1));
}

// E -> R1 = U W V^T, R2 = U W^T V^T (row-major, det +1) and t = u3 (unit), W = [[0, -1, 0], [1, 0, 0], [0, 0, 1]].
// The four decompositions in their fixed order: (R1, +t), (R1, -t), (R2, +t), (R2, -t), of p_b = R p_a + t.
SG_HD bool RelDecompose(const double* E, double* R1, double* R2, double* t) {
  double U[3][3], V[3][3];
  if (!RelSvd2(E, U, V)) return false;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      // U W = [u2, -u1, u3];  U W^T = [-u2, u1, u3]
      const double c = U[i][2] * V[j][2];
      const double s = U[i][1] * V[j][0] - U[i][0] * V[j][1];
      R1[3 * i + j] = s + c;
      R2[3 * i + j] = c - s;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = U[i][2];
  return true;
}

// The depths of d_b f_b = d_a R f_a + t in the least-squares sense (2x2 normal equations, Cramer), f = (x, y, 1).
// g (out) = R f_a.  False when the bearings are parallel (no depths).
SG_HD bool RelDepths(const double* R, const double* t, const double* xa, const double* xb, double* da, double* db,
                     double* g) {
  const double fa[3] = {xa[0], xa[1], 1.0}, fb[3] = {xb[0], xb[1], 1.0};
#pragma unroll
  for (int i = 0; i < 3; ++i) g[i] = pnp_dot(R + 3 * i, fa);
  const double gg = pnp_dot(g, g), gf = pnp_dot(g, fb), ff = pnp_dot(fb, fb);
  const double gt = pnp_dot(g, t), ft = pnp_dot(fb, t);
  const double det = gg * ff - gf * gf;
  if (!(det > 0.0)) return false;
  // [[gg, -gf], [-gf, ff]] [da, db]^T = [-gt, ft]^T
  *da = (-gt * ff + gf * ft) / det;
  *db = (gg * ft - gf * gt) / det;
  return true;
}

// The angle between g = R f_a and f_b = (xb, 1), rad.
SG_HD double RelParallax(const double* g, const double* xb) {
  const double fb[3] = {xb[0], xb[1], 1.0};
  return atan2(sqrt(pnp_cross2(g, fb)), pnp_dot(g, fb));
}

// The decomposition with the most in-front inliers among the four counts, in the fixed order (R1, +t), (R1, -t),
// (R2, +t), (R2, -t); ties go to the earlier.
SG_HD int RelVote(const double* front) {
  int bd = 0;
#pragma unroll
  for (int d = 1; d < 4; ++d)
    if (front[d] > front[bd]) bd = d;
  return bd;
}

// The status of a pair that has a model: the first rule that applies (enum sg_rel_status).  need = max(min_inliers,
// 8); decomposed: RelDecompose succeeded; parallax counts only with min_parallax > 0.
SG_HD int RelStatus(int inliers, int front, int parallax, bool decomposed, int min_inliers, double min_parallax) {
  const int need = min_inliers > kRelSample ? min_inliers : kRelSample;
  if (inliers < need) return SG_REL_FEW_INLIERS;
  if (!decomposed || front < need) return SG_REL_NO_CHEIRALITY;
  if (min_parallax > 0.0 && parallax < need) return SG_REL_LOW_PARALLAX;
  return SG_REL_OK;
}

// (R, t) of p_b = R p_a + t -> q_rel (Eigen [x, y, z, w], unit, w >= 0) and the unit t_rel = -R^T t / |t|, the
// centre of b in a's camera coordinates: p_b = q_rel (p_a - t_rel) up to the unobservable scale.
SG_HD void RelPoseOut(const double* R, const double* t, double* q, double* t_rel) {
  PnpQuatFromRotation(R, q);
  double v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = -(R[c] * t[0] + R[3 + c] * t[1] + R[6 + c] * t[2]);
  const double inv = 1.0 / sqrt(pnp_dot(v, v));
#pragma unroll
  for (int c = 0; c < 3; ++c) t_rel[c] = v[c] * inv;
}

}  // namespace sg

#endif  // SG_RELPOSE_MATH_H_
