// CPU check of csrc/relpose_math.h: the sampler against a table the numpy restatement (tests/relpose_cases.py,
// sample_np) printed and for distinct in-range indices; then, on a case file written by tests/test_relpose_math.py
// from the numpy references (argv[1]): EssentialFromMoments on exact eight-record samples against numpy's estimate up
// to sign, the (1, 1, 0) projection, the Sampson distance against numpy, the decomposition recovering the true
// (R, t); and "no model" for a sample with two identical records and for eight records of one plane.  Built under
// AddressSanitizer and UBSan by that test.  No GPU, no HIP.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "relpose_math.h"

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

// ------------------------------------------------------------------------------------------------ sampler
struct SampleRow {
  uint32_t seed, key;
  int32_t n;
  int32_t idx[3][8];   // h = 0, 255, 1023
};
const SampleRow kTable[] = {
    // TABLE (checked against sample_np by tests/test_relpose_math.py)
    {0u, 262149u, 8, {{2, 3, 1, 7, 0, 4, 6, 5}, {5, 4, 7, 3, 2, 1, 0, 6}, {4, 1, 7, 0, 6, 5, 3, 2}}},
    {0u, 262149u, 9, {{2, 4, 1, 8, 0, 3, 7, 5}, {5, 6, 8, 4, 2, 1, 3, 7}, {4, 1, 8, 2, 7, 6, 5, 0}}},
    {7u, 196616u, 64, {{3, 12, 51, 32, 43, 25, 54, 21}, {51, 42, 2, 63, 61, 31, 25, 62}, {3, 1, 35, 27, 8, 40, 47, 4}}},
    {0u, 262149u, 211, {{61, 90, 43, 193, 18, 20, 183, 44}, {134, 138, 187, 154, 120, 92, 87, 207}, {114, 34, 196, 40, 194, 191, 185, 74}}},
    {3735928559u, 131075u, 5000, {{4771, 2140, 2863, 991, 4702, 1603, 958, 3129}, {4408, 1478, 4895, 4527, 170, 3047, 2778, 2363}, {2913, 2255, 3421, 4349, 895, 1140, 1190, 1668}}},
    // END TABLE
};
const int kTableH[3] = {0, 255, 1023};

void check_sampler() {
  for (const SampleRow& row : kTable)
    for (int j = 0; j < 3; ++j) {
      int32_t idx[8];
      sg::RelSample(row.seed, row.key, kTableH[j], row.n, idx);
      CHECK(std::memcmp(idx, row.idx[j], sizeof(idx)) == 0, "sampler table n %d h %d: %d %d %d %d %d %d %d %d", row.n,
            kTableH[j], idx[0], idx[1], idx[2], idx[3], idx[4], idx[5], idx[6], idx[7]);
    }
  const int ns[5] = {8, 9, 64, 211, 5000};
  for (int n : ns)
    for (uint32_t seed = 0; seed < 3; ++seed)
      for (int h = 0; h < 4096; ++h) {
        int32_t idx[8];
        sg::RelSample(seed, 4u * 65536u + 5u, h, n, idx);
        bool ok = true;
        for (int j = 0; j < 8; ++j) {
          ok = ok && idx[j] >= 0 && idx[j] < n;
          for (int i = 0; i < j; ++i) ok = ok && idx[i] != idx[j];
        }
        CHECK(ok, "sample n %d seed %u h %d not distinct or out of range", n, seed, h);
      }
}

// ------------------------------------------------------------------------------------------------ the case file
bool read(FILE* f, double* v, int n) {
  for (int i = 0; i < n; ++i)
    if (std::fscanf(f, "%lf", &v[i]) != 1) return false;
  return true;
}

double maxdiff_sign(const double* a, const double* b, int n) {
  double dp = 0.0, dm = 0.0;
  for (int i = 0; i < n; ++i) {
    dp = std::fmax(dp, std::fabs(a[i] - b[i]));
    dm = std::fmax(dm, std::fabs(a[i] + b[i]));
  }
  return std::fmin(dp, dm);
}

void check_projection(const double* E, const char* what) {
  // singular values (1, 1, 0)  <=>  E E^T E = E and |E|_F^2 = 2
  double EEt[9], P[9], fro = 0.0, worst = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) EEt[3 * i + j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      P[3 * i + j] = EEt[3 * i] * E[j] + EEt[3 * i + 1] * E[3 + j] + EEt[3 * i + 2] * E[6 + j];
      worst = std::fmax(worst, std::fabs(P[3 * i + j] - E[3 * i + j]));
      fro += E[3 * i + j] * E[3 * i + j];
    }
  CHECK(worst < 1e-13 && std::fabs(fro - 2.0) < 1e-13, "%s: not on the essential manifold (%.3e, |E|^2 %.17g)", what,
        worst, fro);
}

// One pair: n records (xa, xb), intrinsics' inverse focal lengths, the sample, numpy's E and its tolerance, the true
// R and t_rel with their tolerances, a generic matrix with numpy's Sampson distances.
void check_case(FILE* f, int id) {
  double hdr[1];
  if (!read(f, hdr, 1)) return;
  const int n = (int)hdr[0];
  std::vector<double> xa(2 * n), xb(2 * n), s2(n);
  double ifa[2], ifb[2], sidx[8], Enp[9], tol[4], Rt[9], tt[3], Gm[9];
  bool ok = read(f, xa.data(), 2 * n) && read(f, xb.data(), 2 * n) && read(f, ifa, 2) && read(f, ifb, 2) &&
            read(f, sidx, 8) && read(f, Enp, 9) && read(f, tol, 4) && read(f, Rt, 9) && read(f, tt, 3) &&
            read(f, Gm, 9) && read(f, s2.data(), n);
  CHECK(ok, "case %d: short file", id);
  if (!ok) return;
  double sa[8][2], sb[8][2], E[9], gap = 0.0;
  for (int j = 0; j < 8; ++j) {
    const int i = (int)sidx[j];
    sa[j][0] = xa[2 * i]; sa[j][1] = xa[2 * i + 1];
    sb[j][0] = xb[2 * i]; sb[j][1] = xb[2 * i + 1];
  }
  const bool model = sg::RelEightPoint(sa, sb, E, &gap);
  CHECK(model, "case %d: no model, gap %.3e", id, gap);
  if (!model) return;
  const double dE = maxdiff_sign(E, Enp, 9);
  std::printf("case %d: n %d, gap %.3e, |E - E_numpy| %.3e (tolerance %.3e)\n", id, n, gap, dE, tol[0]);
  CHECK(dE <= tol[0], "case %d: E differs from numpy's by %.3e", id, dE);
  check_projection(E, "sample E");
  // Sampson against numpy, on the generic matrix and at E (every record is an exact inlier)
  double worst_rel = 0.0, worst_px = 0.0;
  for (int i = 0; i < n; ++i) {
    const double g = sg::RelSampson(Gm, &xa[2 * i], &xb[2 * i], ifa, ifb);
    worst_rel = std::fmax(worst_rel, std::fabs(g - s2[i]) / s2[i]);
    worst_px = std::fmax(worst_px, std::sqrt(sg::RelSampson(E, &xa[2 * i], &xb[2 * i], ifa, ifb)));
  }
  CHECK(worst_rel < 1e-10, "case %d: Sampson differs from numpy's by %.3e relative", id, worst_rel);
  CHECK(worst_px <= tol[3], "case %d: worst Sampson error %.3e px at the sample's E", id, worst_px);
  // decomposition: the one with the most records in front is the true pose
  double R[2][9], t[3];
  CHECK(sg::RelDecompose(E, R[0], R[1], t), "case %d: no decomposition", id);
  int best = -1, best_front = -1;
  for (int d = 0; d < 4; ++d) {
    const double td[3] = {d & 1 ? -t[0] : t[0], d & 1 ? -t[1] : t[1], d & 1 ? -t[2] : t[2]};
    int front = 0;
    for (int i = 0; i < n; ++i) {
      double da, db, g[3];
      if (sg::RelDepths(R[d >> 1], td, &xa[2 * i], &xb[2 * i], &da, &db, g)) front += da > 0.0 && db > 0.0;
    }
    if (front > best_front) {
      best_front = front;
      best = d;
    }
  }
  CHECK(best_front == n, "case %d: %d of %d records in front", id, best_front, n);
  const double td[3] = {best & 1 ? -t[0] : t[0], best & 1 ? -t[1] : t[1], best & 1 ? -t[2] : t[2]};
  double q[4], tr[3], zero[3] = {0, 0, 0}, Rq[9];
  sg::RelPoseOut(R[best >> 1], td, q, tr);
  for (int c = 0; c < 3; ++c) {   // the quaternion's matrix, column by column
    const double X[4] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0, 1.0};
    double v[3], p[3];
    sg::CameraPoint(q, zero, X, v, p);
    for (int r = 0; r < 3; ++r) Rq[3 * r + c] = p[r];
  }
  double dR = 0.0, dt = 0.0;
  for (int i = 0; i < 9; ++i) dR = std::fmax(dR, std::fabs(Rq[i] - Rt[i]));
  for (int i = 0; i < 3; ++i) dt = std::fmax(dt, std::fabs(tr[i] - tt[i]));
  std::printf("case %d: decomposition %d, |R - R_true| %.3e (%.3e), |t - t_true| %.3e (%.3e), worst Sampson %.3e px\n",
              id, best, dR, tol[1], dt, tol[2], worst_px);
  CHECK(dR <= tol[1] && dt <= tol[2], "case %d: pose off by %.3e / %.3e", id, dR, dt);
  CHECK(std::fabs((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]) - 1.0) < 1e-14 && q[3] >= 0.0,
        "case %d: quaternion norm or sign", id);
  CHECK(std::fabs(tr[0] * tr[0] + tr[1] * tr[1] + tr[2] * tr[2] - 1.0) < 1e-14, "case %d: t_rel not unit", id);
  // two identical records: rank 7, no model
  sa[3][0] = sa[6][0]; sa[3][1] = sa[6][1];
  sb[3][0] = sb[6][0]; sb[3][1] = sb[6][1];
  gap = 1.0;
  CHECK(!sg::RelEightPoint(sa, sb, E, &gap), "case %d: a model from two identical records (gap %.3e)", id, gap);
}

// Eight points of one plane seen by two cameras a sideways step apart: the moment matrix has a three-dimensional
// null space, no model.
void check_plane() {
  double sa[8][2], sb[8][2], E[9], gap = 1.0;
  for (int i = 0; i < 8; ++i) {
    const double X = -1500.0 + 430.0 * i, Y = (i * 37 % 8) * 250.0 - 900.0, Z = 4000.0 + 0.2 * X - 0.1 * Y;
    sa[i][0] = X / Z;
    sa[i][1] = Y / Z;
    sb[i][0] = (X - 150.0) / (Z - 20.0);
    sb[i][1] = Y / (Z - 20.0);
  }
  const bool model = sg::RelEightPoint(sa, sb, E, &gap);
  std::printf("plane: gap %.3e\n", gap);
  CHECK(!model, "a model from eight records of one plane (gap %.3e)", gap);
  for (int i = 0; i < 8; ++i) sa[i][0] = std::nan("");
  CHECK(!sg::RelEightPoint(sa, sb, E, &gap), "a model from NaN records");
}

// The vote's tie rule and every status rule, on hand-built counts.
void check_vote_and_status() {
  const double one[4] = {5, 9, 9, 2}, all[4] = {7, 7, 7, 7}, last[4] = {0, 1, 2, 3}, first[4] = {3, 3, 2, 3};
  CHECK(sg::RelVote(one) == 1, "a tie between 1 and 2 goes to 1");
  CHECK(sg::RelVote(all) == 0, "a four-way tie goes to 0");
  CHECK(sg::RelVote(last) == 3, "the largest wins");
  CHECK(sg::RelVote(first) == 0, "a tie between 0, 1 and 3 goes to 0");
  CHECK(sg::RelStatus(15, 15, 15, true, 16, 0.0) == SG_REL_FEW_INLIERS, "15 inliers of 16");
  CHECK(sg::RelStatus(7, 7, 7, true, 0, 0.0) == SG_REL_FEW_INLIERS, "at least 8 are always required");
  CHECK(sg::RelStatus(8, 8, 0, true, 0, 0.0) == SG_REL_OK, "8 suffice; the parallax gate is off at 0");
  CHECK(sg::RelStatus(40, 15, 15, true, 16, 0.1) == SG_REL_NO_CHEIRALITY, "15 in front of 16");
  CHECK(sg::RelStatus(40, 40, 40, false, 16, 0.0) == SG_REL_NO_CHEIRALITY, "no decomposition");
  CHECK(sg::RelStatus(40, 16, 15, true, 16, 0.1) == SG_REL_LOW_PARALLAX, "15 with the parallax of 16");
  CHECK(sg::RelStatus(40, 16, 16, true, 16, 0.1) == SG_REL_OK, "all rules met");
  CHECK(sg::RelStatus(10, 5, 0, true, 16, 0.1) == SG_REL_FEW_INLIERS, "the first rule that applies");
  // the parallax is an angle in radians between R f_a and f_b
  const double g[3] = {0.0, 0.0, 2.0}, xb[2] = {1.0, 0.0};
  CHECK(std::fabs(sg::RelParallax(g, xb) - 0.7853981633974483) < 1e-15, "45 degrees is pi / 4");
}

}  // namespace

int main(int argc, char** argv) {
  check_sampler();
  check_vote_and_status();
  check_plane();
  if (argc < 2) {
    std::printf("relpose_math_check: no case file\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  double cases[1];
  int n = read(f, cases, 1) ? (int)cases[0] : 0;
  CHECK(n == 4, "%d cases in the file", n);
  for (int i = 0; i < n; ++i) check_case(f, i);
  std::fclose(f);
  if (g_fail) {
    std::printf("relpose_math_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("relpose_math_check OK\n");
  return 0;
}
