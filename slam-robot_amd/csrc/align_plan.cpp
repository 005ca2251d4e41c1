// align_plan.cpp — see align_plan.h.
#include "align_plan.h"

#include <algorithm>
#include <cmath>

#include "common.h"

namespace sg {

namespace {
// TrackedPoint::slam_usable (localmap.h:242-248), as pose_plan.cpp's kPoseUnusableMask
constexpr int kAlignUnusableMask =
    (1 << SG_BAD_LOCATION) | (1 << SG_NO_BASELINE) | (1 << SG_NO_OBSERVATIONS) | (1 << SG_BAD_FEATURE);

// X.xyz / X.w into P; false when a coordinate is not finite or the point is at infinity.
bool Euclidean(const double* X, double* P) {
  for (int c = 0; c < 4; ++c)
    if (!std::isfinite(X[c])) return false;
  // scaled by the largest entry so that the norm neither overflows nor underflows
  const double big = std::max(std::max(std::fabs(X[0]), std::fabs(X[1])), std::max(std::fabs(X[2]), std::fabs(X[3])));
  if (!(big > 0.0)) return false;
  const double x0 = X[0] / big, x1 = X[1] / big, x2 = X[2] / big, x3 = X[3] / big;
  const double norm = std::sqrt((x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3));
  if (!(std::fabs(x3) >= kAlignMinW * norm)) return false;
  for (int c = 0; c < 3; ++c) P[c] = X[c] / X[3];
  return true;
}
}  // namespace

void PlanAlign(const sg_map* mp, const int32_t* corr, const int32_t* group_offset, int32_t n,
               const sg_align_options* o, AlignPlan* out) {
  SG_REQUIRE(mp && o && out, SG_EINVAL, "null argument");
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative group count");
  SG_REQUIRE(o->threshold > 0.0, SG_EINVAL, "threshold must be positive");
  SG_REQUIRE(o->max_hypotheses > 0, SG_EINVAL, "max_hypotheses must be positive");
  SG_REQUIRE(o->min_gap >= 0.0, SG_EINVAL, "min_gap must not be negative");
  SG_REQUIRE(o->max_scale == 0.0 || o->max_scale >= 1.0, SG_EINVAL, "max_scale must be 0 or at least 1");
  SG_REQUIRE(n == 0 || group_offset, SG_EINVAL, "null group offsets");
  const sg_map& m = *mp;
  SG_REQUIRE(m.num_points >= 0, SG_EINVAL, "negative map sizes");
  const int P = m.num_points;
  out->H = (std::min(o->max_hypotheses, kAlignMaxHypotheses) + kAlignThreads - 1) / kAlignThreads * kAlignThreads;
  out->S = out->H / kAlignThreads;
  out->grid = (int64_t)n * out->S;
  SG_REQUIRE(out->grid <= 0x7fffffff, SG_EINVAL, "too many groups for this many hypotheses");
  out->off.assign((size_t)n + 1, 0);
  out->records.clear();
  out->rec_corr.clear();
  out->groups.assign((size_t)n, AlignGroup{});
  out->num_run = 0;
  if (n == 0) return;
  SG_REQUIRE(group_offset[0] == 0, SG_EINVAL, "group_offset[0] must be 0");
  for (int g = 0; g < n; ++g)
    SG_REQUIRE(group_offset[g + 1] >= group_offset[g], SG_EINVAL, "decreasing group offset");
  const int32_t total = group_offset[n];
  SG_REQUIRE(total == 0 || corr, SG_EINVAL, "null correspondence list");
  SG_REQUIRE(total == 0 || (m.X && m.point_flags), SG_EINVAL, "the map's points cannot be read");
  for (int32_t j = 0; j < total; ++j) {
    const int a = corr[2 * (size_t)j], b = corr[2 * (size_t)j + 1];
    SG_REQUIRE(a >= 0 && a < P && b >= 0 && b < P, SG_EINVAL, "point index out of range");
    SG_REQUIRE(a != b, SG_EINVAL, "a correspondence of one point");
  }
  for (int g = 0; g < n; ++g) {
    AlignGroup& ag = out->groups[g];
    ag.num_corr = group_offset[g + 1] - group_offset[g];
    ag.key = ag.num_corr > 0 ? corr[2 * (size_t)group_offset[g]] : 0;
    for (int32_t j = group_offset[g]; j < group_offset[g + 1]; ++j) {
      const int a = corr[2 * (size_t)j], b = corr[2 * (size_t)j + 1];
      if ((m.point_flags[a] & kAlignUnusableMask) != 0 || (m.point_flags[b] & kAlignUnusableMask) != 0) continue;
      double rec[6];
      if (!Euclidean(m.X + 4 * (size_t)a, rec) || !Euclidean(m.X + 4 * (size_t)b, rec + 3)) continue;
      out->records.insert(out->records.end(), rec, rec + 6);
      out->rec_corr.push_back(j);
    }
    out->off[g + 1] = (int32_t)out->rec_corr.size();
    ag.run = out->off[g + 1] - out->off[g] >= kAlignMinRecords;
    out->num_run += ag.run;
  }
}

}  // namespace sg
