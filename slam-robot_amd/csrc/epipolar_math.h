// epipolar_math.h — the arithmetic of sg_slam_match_epipolar ("which keypoint of frame b can be the keypoint of frame a,
// given both poses"), device code that also compiles on the host: k_epi_prep and k_epi_window (ba_epipolar.hip), the
// planner's CPU executor (epipolar_plan.cpp) and the CPU check (tests/native/epipolar_plan_check.cpp) run this one copy.
//
//   EpiPairFrom    two stored poses and their cameras -> the pair record: R = R_b R_a^T, tr = R_b (t_a - t_b),
//                  E = [tr]x R (row-major, x_b^T E x_a = 0 on plane coordinates), the inverse focal lengths, and
//                  whether the pair is degenerate.  The map's convention p = R(q) (X - t W), R(q) the matrix of
//                  ProjectJacobian (project_math.h), the quaternion not normalised;
//   EpiPrepA/B     one keypoint -> everything of the three tests that depends on that keypoint alone.  The 8-step
//                  Newton undistortion runs here, once per keypoint;
//   EpiGate        RelSampson (relpose_math.h) <= tol^2 4^L without the division, from the two records;
//   EpiDepth       the signs of RelDepths' det and of its two numerators;
//   EpiParallax    RelParallax of the two bearings against the threshold;
//   EpiCandidate   the three in the contract's order.
// Every comparison is false on a NaN.
#ifndef SG_EPIPOLAR_MATH_H_
#define SG_EPIPOLAR_MATH_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // (project_math.h's SG_HD needs it where hipcc builds a host-only file)
#endif

#include "pnp_math.h"
#include "project_math.h"
#include "relpose_math.h"

namespace sg {

struct EpiPair {
  double E[9], R[9], tr[3];
  double ifa[2], ifb[2];   // {1 / fx, 1 / fy} of frame a's and frame b's camera
  double ka[7], kb[7];     // the two cameras' intrinsics
  int32_t degenerate;      // an entry of E, R or tr is not finite, or E is all zero: the pair has no candidates
  int32_t pad;
};
static_assert(sizeof(EpiPair) == 320, "read by k_epi_prep as 39 doubles and two ints");

struct EpiA {
  double x[2];    // plane coordinates
  double l[3];    // E (x, 1): the epipolar line in b
  double na;      // (l0 ifb0)^2 + (l1 ifb1)^2
  double g[3];    // R (x, 1): the bearing in b's axes
  double gg, gt;  // g . g, g . tr
  double scale;   // 4^level
};
static_assert(sizeof(EpiA) == 96, "held by one lane of k_epi_window as 12 doubles");

struct EpiB {
  double x[2];    // plane coordinates
  double nb;      // (m0 ifa0)^2 + (m1 ifa1)^2 with m = E^T (x, 1)
  double scale;   // 4^level
  double ff, ft;  // f . f and f . tr with f = (x, 1)
};
static_assert(sizeof(EpiB) == 48, "staged in LDS by k_epi_window as 6 doubles");

// The rotation matrix of a stored quaternion (Eigen memory [x, y, z, w]), row-major: project_math.h:125-133.
SG_HD void EpiRotation(const double* q, double* R) {
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

SG_HD void EpiPairFrom(const double* qa, const double* ta, const double* ka, const double* qb, const double* tb,
                       const double* kb, EpiPair* p) {
  double Ra[9], Rb[9];
  EpiRotation(qa, Ra);
  EpiRotation(qb, Rb);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) p->R[3 * i + j] = pnp_dot(Rb + 3 * i, Ra + 3 * j);   // R_b R_a^T
  const double d[3] = {ta[0] - tb[0], ta[1] - tb[1], ta[2] - tb[2]};
  for (int i = 0; i < 3; ++i) p->tr[i] = pnp_dot(Rb + 3 * i, d);
  const double* t = p->tr;
  for (int j = 0; j < 3; ++j) {   // [tr]x R, column by column
    const double c[3] = {p->R[j], p->R[3 + j], p->R[6 + j]};
    double e[3];
    pnp_cross(t, c, e);
    p->E[j] = e[0];
    p->E[3 + j] = e[1];
    p->E[6 + j] = e[2];
  }
  p->ifa[0] = 1.0 / ka[3];
  p->ifa[1] = 1.0 / ka[4];
  p->ifb[0] = 1.0 / kb[3];
  p->ifb[1] = 1.0 / kb[4];
  for (int i = 0; i < 7; ++i) {
    p->ka[i] = ka[i];
    p->kb[i] = kb[i];
  }
  bool finite = true, zero = true;
  for (int i = 0; i < 9; ++i) {
    finite = finite && PnpFinite(p->E[i]) && PnpFinite(p->R[i]);
    zero = zero && p->E[i] == 0.0;
  }
  for (int i = 0; i < 3; ++i) finite = finite && PnpFinite(p->tr[i]);
  p->degenerate = (!finite || zero) ? 1 : 0;
  p->pad = 0;
}

SG_HD double EpiLevelScale(int level) { return (double)(1u << (2 * level)); }   // 4^level, level in 0..7

SG_HD void EpiPrepA(const EpiPair& p, const double* pixel, int level, EpiA* a) {
  UndistortPixel(p.ka, pixel, a->x);
  const double f[3] = {a->x[0], a->x[1], 1.0};
  for (int i = 0; i < 3; ++i) {
    a->l[i] = pnp_dot(p.E + 3 * i, f);
    a->g[i] = pnp_dot(p.R + 3 * i, f);
  }
  const double a0 = a->l[0] * p.ifb[0], a1 = a->l[1] * p.ifb[1];
  a->na = a0 * a0 + a1 * a1;
  a->gg = pnp_dot(a->g, a->g);
  a->gt = pnp_dot(a->g, p.tr);
  a->scale = EpiLevelScale(level);
}

SG_HD void EpiPrepB(const EpiPair& p, const double* pixel, int level, EpiB* b) {
  UndistortPixel(p.kb, pixel, b->x);
  const double f[3] = {b->x[0], b->x[1], 1.0};
  const double m0 = p.E[0] * f[0] + p.E[3] * f[1] + p.E[6];
  const double m1 = p.E[1] * f[0] + p.E[4] * f[1] + p.E[7];
  const double b0 = m0 * p.ifa[0], b1 = m1 * p.ifa[1];
  b->nb = b0 * b0 + b1 * b1;
  b->scale = EpiLevelScale(level);
  b->ff = pnp_dot(f, f);
  b->ft = pnp_dot(f, p.tr);
}

// A record that is no candidate of any keypoint: r is NaN, so the gate's comparison is false whatever the a side
// holds.  k_epi_window pads the tail of a tile with it.
SG_HD EpiB EpiPadB() {
  EpiB b;
  b.x[0] = b.x[1] = NAN;
  b.nb = INFINITY;
  b.scale = 1.0;
  b.ff = b.ft = NAN;
  return b;
}

// r^2 <= tol^2 4^L (na + nb) with r = x_b . l and L the larger of the two levels; tol2 = tol_px^2.
SG_HD bool EpiGate(const EpiA& a, const EpiB& b, double tol2) {
  const double r = b.x[0] * a.l[0] + b.x[1] * a.l[1] + a.l[2];
  const double den = a.na + b.nb;
  const double s = a.scale > b.scale ? a.scale : b.scale;
  return den > 0.0 && r * r <= tol2 * s * den;
}

// Both depths of d_b f_b = d_a g + tr positive: RelDepths' det and its two numerators, signs only.
SG_HD bool EpiDepth(const EpiA& a, const EpiB& b) {
  const double f[3] = {b.x[0], b.x[1], 1.0};
  const double gf = pnp_dot(a.g, f);
  const double det = a.gg * b.ff - gf * gf;
  const double da = -a.gt * b.ff + gf * b.ft;
  const double db = a.gg * b.ft - gf * a.gt;
  return det > 0.0 && da > 0.0 && db > 0.0;
}

SG_HD bool EpiParallax(const EpiA& a, const EpiB& b, double min_parallax) {
  return RelParallax(a.g, b.x) >= min_parallax;
}

// Step 3 of the contract, in its order.  min_parallax == 0: no parallax test.
SG_HD bool EpiCandidate(const EpiA& a, const EpiB& b, double tol2, double min_parallax) {
  if (!EpiGate(a, b, tol2)) return false;
  if (!EpiDepth(a, b)) return false;
  return !(min_parallax > 0.0) || EpiParallax(a, b, min_parallax);
}

}  // namespace sg

#endif  // SG_EPIPOLAR_MATH_H_
