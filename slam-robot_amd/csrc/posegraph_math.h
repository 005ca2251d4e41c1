// posegraph_math.h — the arithmetic of sg_slam_optimize_pose_graph shared by the device (ba_posegraph.hip) and the
// host (posegraph_plan.cpp's CPU executor, tests/native/posegraph_math_check.cpp): the residual of one pose-graph
// edge with its analytic 7 x 14 Jacobian, and the per-entry steps of the planned sparse block Cholesky.  Every
// function does the work of ONE item (an edge, a matrix entry, a row); the device strides them over a workgroup,
// the host loops over them, so both follow the same arithmetic.
//
// Node state x[8]: q (Eigen memory [x, y, z, w], unit, the map's p = R(q)(X - t)) | t (camera centre) | sigma (log
// of the local map scale; world-from-camera is p -> e^sigma R^T p + t).  Free nodes carry D = 7 unknowns, rotation
// by ceres::QuaternionParameterization as project_math.h applies it (QuatPlus, QuatLocalJacobian), t and sigma
// additive; with fix_scale D = 6, sigma stays 0 and the scale residual is dropped.
//
// Edge (a, b) with measurement q^ | u^ | rho^ and weights w_rot, w_t, w_s:
//   q_e = conj(q^) (x) q_a (x) conj(q_b), sign-flipped to w >= 0;  omega = its rotation vector
//   r[0:3] = w_rot omega,   r[3:6] = w_t (e^-sigma_a R_a (t_b - t_a) - u^),   r[6] = w_s (sigma_b - sigma_a - rho^)
// omega = 2 atan2(|v|, w) v / |v|; for |v|^2 < kPgSeriesTheta2 the factor 2 atan2(|v|, w) / |v| and its derivative
// come from the series in x = |v| / w (the terms left out are below 1e-25 relative).
#ifndef SG_POSEGRAPH_MATH_H_
#define SG_POSEGRAPH_MATH_H_

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // (project_math.h's SG_HD needs it where hipcc builds a host-only file)
#endif

#include "project_math.h"

namespace sg {

constexpr double kPgSeriesTheta2 = 1e-8;   // |v|^2 of q_e below which the series is used
constexpr int kPgRes = 7;                  // residuals per edge (the 7th is zero with fix_scale)
constexpr int kPgCols = 14;                // Jacobian columns: a's rot 3 | t 3 | sigma, then b's
constexpr int kPgRec = kPgRes + kPgRes * kPgCols;   // an edge's stored record: r~ (7) | J~ (7 x 14, row-major)
constexpr int kPgState = 8;                // q 4 | t 3 | sigma
constexpr int kPgBlk = 49;                 // doubles of one block of L (7 x 7, row-major; D x D of it are used)

// Hamilton product on Eigen memory [x, y, z, w]: the rotation of b, then that of a.
SG_HD void PgQuatMul(const double* a, const double* b, double* o) {
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
  o[2] = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
}
SG_HD void PgCross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
// p = R(q) d by Eigen's _transformVector, as CameraPoint does.
SG_HD void PgRotate(const double* q, const double* d, double* p) {
  double c[3], e[3];
  PgCross(q, d, c);
  c[0] += c[0]; c[1] += c[1]; c[2] += c[2];
  PgCross(q, c, e);
  for (int i = 0; i < 3; ++i) p[i] = (d[i] + q[3] * c[i]) + e[i];
}
// The derivative of R(q) d along the quaternion direction dq (4): 2 dw (v x d) + 2 w (dv x d) + 2 (dv x (v x d) +
// v x (dv x d)), v the vector part of q.
SG_HD void PgRotateDq(const double* q, const double* d, const double* dq, double* dp) {
  double vd[3], dvd[3], a[3], b[3];
  PgCross(q, d, vd);
  PgCross(dq, d, dvd);
  PgCross(dq, vd, a);
  PgCross(q, dvd, b);
  for (int i = 0; i < 3; ++i) dp[i] = 2.0 * (dq[3] * vd[i] + q[3] * dvd[i] + (a[i] + b[i]));
}

// The rotation vector of the quaternion e (w >= 0) and the factors of its derivative:
//   omega = g v,   d omega / d v = g I + h v v^T,   d omega / d w = dw v.
SG_HD void PgLogFactors(const double* e, double* g, double* h, double* dw) {
  const double th2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
  const double w = e[3];
  const double n2 = th2 + w * w;
  *dw = -2.0 / n2;
  if (th2 < kPgSeriesTheta2) {
    const double x2 = th2 / (w * w);
    *g = (2.0 / w) * (1.0 - x2 * (1.0 / 3.0 - x2 * 0.2));
    *h = (2.0 / (w * w * w)) * (-2.0 / 3.0 + 0.8 * x2);
  } else {
    const double th = sqrt(th2);
    *g = 2.0 * atan2(th, w) / th;
    *h = (2.0 * w / n2 - *g) / th2;
  }
}

// One edge at the states xa, xb (kPgState doubles each).  meas: q^ 4 | u^ 3 | rho^; w: w_rot, w_t, w_s.  b > 0:
// CauchyLoss with b = range^2 on s = |r|^2; b == 0: no loss.  Writes the corrected residual r~ = sqrt(rho') r into
// rec[0 .. 6] and, with jac, the corrected Jacobian sqrt(rho') J into rec[7 ..] (7 x 14, row-major; with fix_scale
// row 6 and columns 6 and 13 are zero).  rec may be global memory: every entry is written once and none is read.
// Returns the cost 0.5 rho(s); *rho1 (may be null) receives rho'.
SG_HD double PgEdgeEval(const double* xa, const double* xb, const double* meas, const double* w, int fix_scale, double b,
                        double inv_b, bool jac, double* rec, double* rho1) {
  const double ch[4] = {-meas[0], -meas[1], -meas[2], meas[3]};   // conj(q^)
  const double cb[4] = {-xb[0], -xb[1], -xb[2], xb[3]};           // conj(q_b)
  double m[4], e[4];
  PgQuatMul(ch, xa, m);   // conj(q^) (x) q_a
  PgQuatMul(m, cb, e);
  const double sgn = e[3] < 0.0 ? -1.0 : 1.0;
  for (int i = 0; i < 4; ++i) e[i] *= sgn;
  double g, h, dw;
  PgLogFactors(e, &g, &h, &dw);
  const double d[3] = {xb[4] - xa[4], xb[5] - xa[5], xb[6] - xa[6]};
  double p[3];
  PgRotate(xa, d, p);
  const double es = fix_scale ? 1.0 : exp(-xa[7]);
  const double ws = fix_scale ? 0.0 : w[2];
  double r[kPgRes];
  for (int i = 0; i < 3; ++i) {
    r[i] = w[0] * (g * e[i]);
    r[3 + i] = w[1] * (es * p[i] - meas[4 + i]);
  }
  r[6] = fix_scale ? 0.0 : ws * ((xb[7] - xa[7]) - meas[7]);
  double s = 0.0;
  for (int i = 0; i < kPgRes; ++i) s += r[i] * r[i];
  double rho0 = s, r1 = 1.0;
  if (b > 0.0) Cauchy(s, b, inv_b, &rho0, &r1);
  const double sr = sqrt(r1);
  for (int i = 0; i < kPgRes; ++i) rec[i] = sr * r[i];
  if (rho1) *rho1 = r1;
  if (!jac) return 0.5 * rho0;
  double* J = rec + kPgRes;
  const double wr = sr * w[0], wt = sr * w[1];
  double La[12], Lb[12];
  QuatLocalJacobian(xa, La);
  QuatLocalJacobian(xb, Lb);
  for (int k = 0; k < 3; ++k) {
    // rotation columns: the direction of q_e along local coordinate k of a, then of b (q_e is linear in q_a and q_b)
    const double da[4] = {La[k], La[3 + k], La[6 + k], La[9 + k]};
    const double dbc[4] = {-Lb[k], -Lb[3 + k], -Lb[6 + k], Lb[9 + k]};   // conj of b's direction
    double t4[4], ea[4], eb[4];
    PgQuatMul(ch, da, t4);
    PgQuatMul(t4, cb, ea);
    PgQuatMul(m, dbc, eb);
    const double va = sgn * (e[0] * ea[0] + e[1] * ea[1] + e[2] * ea[2]);
    const double vb = sgn * (e[0] * eb[0] + e[1] * eb[1] + e[2] * eb[2]);
    double dpa[3];
    PgRotateDq(xa, d, da, dpa);
    for (int i = 0; i < 3; ++i) {
      J[i * kPgCols + k] = wr * (g * (sgn * ea[i]) + h * va * e[i] + dw * (sgn * ea[3]) * e[i]);
      J[i * kPgCols + 7 + k] = wr * (g * (sgn * eb[i]) + h * vb * e[i] + dw * (sgn * eb[3]) * e[i]);
      J[(3 + i) * kPgCols + k] = wt * es * dpa[i];
      J[(3 + i) * kPgCols + 7 + k] = 0.0;
    }
    J[6 * kPgCols + k] = 0.0;
    J[6 * kPgCols + 7 + k] = 0.0;
    // translation columns: e^-sigma_a R_a on t_b, its negative on t_a; R_a's column k is R_a applied to unit k
    double uk[3] = {0.0, 0.0, 0.0}, rc[3];
    uk[k] = 1.0;
    PgRotate(xa, uk, rc);
    for (int i = 0; i < 3; ++i) {
      J[i * kPgCols + 3 + k] = 0.0;
      J[i * kPgCols + 10 + k] = 0.0;
      J[(3 + i) * kPgCols + 3 + k] = -(wt * es * rc[i]);
      J[(3 + i) * kPgCols + 10 + k] = wt * es * rc[i];
    }
    J[6 * kPgCols + 3 + k] = 0.0;
    J[6 * kPgCols + 10 + k] = 0.0;
  }
  for (int i = 0; i < 3; ++i) {
    J[i * kPgCols + 6] = 0.0;
    J[i * kPgCols + 13] = 0.0;
    J[(3 + i) * kPgCols + 6] = fix_scale ? 0.0 : -(wt * es * p[i]);
    J[(3 + i) * kPgCols + 13] = 0.0;
  }
  J[6 * kPgCols + 6] = -(sr * ws);
  J[6 * kPgCols + 13] = sr * ws;
  return 0.5 * rho0;
}

// ------------------------------------------------------------------------------------------------------------------
// The planned problem as the kernels and the CPU executor read it (posegraph_plan.h fills it; all arrays are
// call-wide, a graph's share is named by the offsets of its PgGraph).
struct PgGraph {
  int32_t run;          // 1: solved on the device; 0: SG_PG_DID_NOT_RUN or SG_PG_NO_ANCHOR (no workgroup work)
  int32_t node0, nn;    // its nodes: node0 .. node0 + nn
  int32_t edge0, ne;    // its edges
  int32_t col0, nc;     // its columns (free nodes in elimination order)
  int32_t blk0, nb;     // its blocks of L
  int32_t status;       // enum sg_posegraph_status as decided on the host
  int32_t pad[2];
};
static_assert(sizeof(PgGraph) == 48, "read by k_posegraph_lm as 12 ints");

struct PgView {
  const PgGraph* graphs;
  const int32_t* node_col;     // [nodes] local column of the node, -1 when fixed
  const int32_t* col_node;     // [cols] local node of the column
  const int32_t* edge_ab;      // [2 edges] local nodes a, b
  const double* edge_meas;     // [8 edges]
  const double* edge_w;        // [3 edges]
  // L: lower block pattern, column-major; column j's blocks are colptr[j] .. colptr[j + 1], the diagonal first, then
  // ascending rows
  const int32_t* colptr;       // [cols + 1] call-wide block index
  const int32_t* blk_row;      // [blocks] local column index of the block's row
  const int32_t* blk_col;      // [blocks] of its column
  const int32_t* asm_ptr;      // [blocks + 1] the block's contributions in listed edge order
  const int32_t* asm_items;    // 4 * local edge + code: 0 Ja^T Ja, 1 Jb^T Jb, 2 Ja^T Jb, 3 Jb^T Ja
  const int32_t* gasm_ptr;     // [cols + 1] the gradient segment's contributions in listed edge order
  const int32_t* gasm_items;   // 2 * local edge + side
  const int32_t* upd_ptr;      // [cols + 1] the column's update triples
  const int32_t* upd;          // 3 per triple: block L_ij, block L_kj, target block (i, k); call-wide block indices
  double* L;                   // [kPgBlk blocks]
  double* rec[2];              // [kPgRec edges] the linearization at x[slot]
  double* x[2];                // [kPgState nodes]
  double *g, *hd, *scale, *diag, *y, *delta;   // [7 cols]
  int32_t D, fix_scale;        // 7 / 0 or 6 / 1
  double b, inv_b;             // CauchyLoss(range): b = range^2; 0: no loss
};

// Entry i of graph G's gradient: column i / D, component i % D.  g = sum J_side^T r~ and hd = the diagonal of J^T J.
SG_HD void PgGradEntry(const PgView& v, const PgGraph& G, int i, int slot) {
  const int j = i / v.D, k = i - j * v.D;
  const int c = G.col0 + j;
  double gs = 0.0, hs = 0.0;
  for (int it = v.gasm_ptr[c]; it < v.gasm_ptr[c + 1]; ++it) {
    const int item = v.gasm_items[it];
    const double* R = v.rec[slot] + (size_t)kPgRec * (G.edge0 + (item >> 1));
    const double* Jc = R + kPgRes + 7 * (item & 1) + k;
    for (int r = 0; r < kPgRes; ++r) {
      const double a = Jc[r * kPgCols];
      gs += a * R[r];
      hs += a * a;
    }
  }
  v.g[7 * (size_t)c + k] = gs;
  v.hd[7 * (size_t)c + k] = hs;
}

// Entry i of graph G's damped, Jacobi-scaled normal matrix in L's pattern: block i / D^2, row r, column c of it.
SG_HD void PgAssembleEntry(const PgView& v, const PgGraph& G, int i, int slot, double radius) {
  const int dd = v.D * v.D;
  const int bl = i / dd, rc = i - bl * dd;
  const int r = rc / v.D, c = rc - r * v.D;
  const int B = G.blk0 + bl;
  double s = 0.0;
  for (int it = v.asm_ptr[B]; it < v.asm_ptr[B + 1]; ++it) {
    const int item = v.asm_items[it], code = item & 3;
    const double* J = v.rec[slot] + (size_t)kPgRec * (G.edge0 + (item >> 2)) + kPgRes;
    const double* Jr = J + ((code == 0 || code == 2) ? 0 : 7) + r;
    const double* Jc = J + ((code == 0 || code == 3) ? 0 : 7) + c;
    for (int q = 0; q < kPgRes; ++q) s += Jr[q * kPgCols] * Jc[q * kPgCols];
  }
  const size_t row = 7 * (size_t)(G.col0 + v.blk_row[B]), col = 7 * (size_t)(G.col0 + v.blk_col[B]);
  s *= v.scale[row + r] * v.scale[col + c];
  if (row == col && r == c) s += v.diag[row + r] / radius;
  v.L[(size_t)kPgBlk * B + 7 * r + c] = s;
}

// Column j's diagonal block: in-place lower Cholesky (the strict upper part is not read afterwards).  False on a
// non-positive (or NaN) pivot: the step is invalid.
SG_HD bool PgFactorDiag(const PgView& v, const PgGraph& G, int j) {
  double* A = v.L + (size_t)kPgBlk * v.colptr[G.col0 + j];
  const int D = v.D;
  for (int c = 0; c < D; ++c) {
    double d = A[7 * c + c];
    for (int k = 0; k < c; ++k) d -= A[7 * c + k] * A[7 * c + k];
    if (!(d > 0.0)) return false;
    const double l = sqrt(d), inv = 1.0 / l;
    A[7 * c + c] = l;
    for (int i = c + 1; i < D; ++i) {
      double t = A[7 * i + c];
      for (int k = 0; k < c; ++k) t -= A[7 * i + k] * A[7 * c + k];
      A[7 * i + c] = t * inv;
    }
  }
  return true;
}
// Item i of column j's off-diagonal solves: row i % D of its off-diagonal block 1 + i / D, X L_jj^T = A in place.
SG_HD void PgSolveOffRow(const PgView& v, const PgGraph& G, int j, int i) {
  const int D = v.D, b0 = v.colptr[G.col0 + j];
  const double* Ljj = v.L + (size_t)kPgBlk * b0;
  double* X = v.L + (size_t)kPgBlk * (b0 + 1 + i / D) + 7 * (i % D);
  for (int c = 0; c < D; ++c) {
    double t = X[c];
    for (int k = 0; k < c; ++k) t -= X[k] * Ljj[7 * c + k];
    X[c] = t / Ljj[7 * c + c];
  }
}
// Item i of column j's updates: entry i % D^2 of the target of triple i / D^2, target -= L_ij L_kj^T.
SG_HD void PgUpdateEntry(const PgView& v, const PgGraph& G, int j, int i) {
  const int D = v.D, dd = D * D;
  const int u = v.upd_ptr[G.col0 + j] + i / dd, rc = i % dd;
  const int r = rc / D, c = rc - r * D;
  const double* Li = v.L + (size_t)kPgBlk * v.upd[3 * (size_t)u] + 7 * r;
  const double* Lk = v.L + (size_t)kPgBlk * v.upd[3 * (size_t)u + 1] + 7 * c;
  double s = 0.0;
  for (int k = 0; k < D; ++k) s += Li[k] * Lk[k];
  v.L[(size_t)kPgBlk * v.upd[3 * (size_t)u + 2] + 7 * r + c] -= s;
}
// Forward substitution, column j: y_j <- L_jj^-1 y_j (one item), then item i of its rows: y_row -= L_row,j y_j.
SG_HD void PgForwardDiag(const PgView& v, const PgGraph& G, int j) {
  const int D = v.D;
  const double* Ljj = v.L + (size_t)kPgBlk * v.colptr[G.col0 + j];
  double* y = v.y + 7 * (size_t)(G.col0 + j);
  for (int r = 0; r < D; ++r) {
    double t = y[r];
    for (int k = 0; k < r; ++k) t -= Ljj[7 * r + k] * y[k];
    y[r] = t / Ljj[7 * r + r];
  }
}
SG_HD void PgForwardRow(const PgView& v, const PgGraph& G, int j, int i) {
  const int D = v.D, B = v.colptr[G.col0 + j] + 1 + i / D, r = i % D;
  const double* Lr = v.L + (size_t)kPgBlk * B + 7 * r;
  const double* yj = v.y + 7 * (size_t)(G.col0 + j);
  double s = 0.0;
  for (int k = 0; k < D; ++k) s += Lr[k] * yj[k];
  v.y[7 * (size_t)(G.col0 + v.blk_row[B]) + r] -= s;
}
// Back substitution, column j: component c of y_j -= sum over its rows of L_row,j^T y_row (D items), then
// y_j <- L_jj^-T y_j (one item).
SG_HD void PgBackwardGather(const PgView& v, const PgGraph& G, int j, int c) {
  const int D = v.D, b0 = v.colptr[G.col0 + j], b1 = v.colptr[G.col0 + j + 1];
  double s = 0.0;
  for (int B = b0 + 1; B < b1; ++B) {
    const double* Lb = v.L + (size_t)kPgBlk * B + c;
    const double* yr = v.y + 7 * (size_t)(G.col0 + v.blk_row[B]);
    for (int r = 0; r < D; ++r) s += Lb[7 * r] * yr[r];
  }
  v.y[7 * (size_t)(G.col0 + j) + c] -= s;
}
SG_HD void PgBackwardDiag(const PgView& v, const PgGraph& G, int j) {
  const int D = v.D;
  const double* Ljj = v.L + (size_t)kPgBlk * v.colptr[G.col0 + j];
  double* y = v.y + 7 * (size_t)(G.col0 + j);
  for (int r = D - 1; r >= 0; --r) {
    double t = y[r];
    for (int k = r + 1; k < D; ++k) t -= Ljj[7 * k + r] * y[k];
    y[r] = t / Ljj[7 * r + r];
  }
}

// Node nd's candidate: delta = -scale y on its column (nothing for a fixed node), x[cur ^ 1] = x[cur] (+) delta.
// sums[0] += |x_cand - x|^2, sums[1] += |x_cand|^2 over the node's free parameters (q 4, t 3, and sigma unless
// fix_scale), as Ceres counts them.
SG_HD void PgCandidateNode(const PgView& v, const PgGraph& G, int nd, int cur, double* sums) {
  const double* x = v.x[cur] + kPgState * (size_t)(G.node0 + nd);
  double* xc = v.x[cur ^ 1] + kPgState * (size_t)(G.node0 + nd);
  const int j = v.node_col[G.node0 + nd];
  if (j < 0) {
    for (int i = 0; i < kPgState; ++i) xc[i] = x[i];
    return;
  }
  const size_t c = 7 * (size_t)(G.col0 + j);
  double dl[7];
  for (int i = 0; i < 7; ++i) dl[i] = i < v.D ? -(v.y[c + i] * v.scale[c + i]) : 0.0;
  for (int i = 0; i < 7; ++i) v.delta[c + i] = dl[i];
  double o[kPgState];
  QuatPlus(x, dl, o);
  for (int i = 0; i < 3; ++i) o[4 + i] = x[4 + i] + dl[3 + i];
  o[7] = x[7] + dl[6];
  const int np = v.fix_scale ? 7 : 8;
  for (int i = 0; i < kPgState; ++i) xc[i] = o[i];
  for (int i = 0; i < np; ++i) {
    sums[0] += (x[i] - o[i]) * (x[i] - o[i]);
    sums[1] += o[i] * o[i];
  }
}
SG_HD double PgNodeNorm2(const PgView& v, const PgGraph& G, int nd, int slot) {
  if (v.node_col[G.node0 + nd] < 0) return 0.0;
  const double* x = v.x[slot] + kPgState * (size_t)(G.node0 + nd);
  const int np = v.fix_scale ? 7 : 8;
  double s = 0.0;
  for (int i = 0; i < np; ++i) s += x[i] * x[i];
  return s;
}
// Edge e's share of the model cost change, -(J~ delta) . (r~ + J~ delta / 2), from the stored record.
SG_HD double PgModelEdge(const PgView& v, const PgGraph& G, int e, int cur) {
  const double* R = v.rec[cur] + (size_t)kPgRec * (G.edge0 + e);
  const int ja = v.node_col[G.node0 + v.edge_ab[2 * (size_t)(G.edge0 + e)]];
  const int jb = v.node_col[G.node0 + v.edge_ab[2 * (size_t)(G.edge0 + e) + 1]];
  if (ja < 0 && jb < 0) return 0.0;
  const double* da = ja >= 0 ? v.delta + 7 * (size_t)(G.col0 + ja) : nullptr;
  const double* db = jb >= 0 ? v.delta + 7 * (size_t)(G.col0 + jb) : nullptr;
  double m = 0.0;
  for (int r = 0; r < kPgRes; ++r) {
    const double* J = R + kPgRes + r * kPgCols;
    double jd = 0.0;
    if (da)
      for (int k = 0; k < v.D; ++k) jd += J[k] * da[k];
    if (db)
      for (int k = 0; k < v.D; ++k) jd += J[7 + k] * db[k];
    m += jd * (R[r] + 0.5 * jd);
  }
  return -m;
}
// Edge e linearized at x[slot] into rec[slot]; returns its cost.  *fixed: the edge joins two fixed nodes (its cost
// belongs to fixed_cost, and its record is never read).
SG_HD double PgEdgeLinearize(const PgView& v, const PgGraph& G, int e, int slot, bool* fixed) {
  const size_t E = (size_t)(G.edge0 + e);
  const int a = v.edge_ab[2 * E], b = v.edge_ab[2 * E + 1];
  *fixed = v.node_col[G.node0 + a] < 0 && v.node_col[G.node0 + b] < 0;
  return PgEdgeEval(v.x[slot] + kPgState * (size_t)(G.node0 + a), v.x[slot] + kPgState * (size_t)(G.node0 + b),
                    v.edge_meas + 8 * E, v.edge_w + 3 * E, v.fix_scale, v.b, v.inv_b, !*fixed, v.rec[slot] + kPgRec * E,
                    nullptr);
}

}  // namespace sg

#endif  // SG_POSEGRAPH_MATH_H_
