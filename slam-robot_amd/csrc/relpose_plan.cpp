// relpose_plan.cpp — see relpose_plan.h.
#include "relpose_plan.h"

#include <algorithm>
#include <cstring>

#include "common.h"

namespace sg {

void PlanRelPoses(const sg_map* mp, const int32_t* pairs, int32_t n, const sg_relpose_options* o, RelPlan* out) {
  SG_REQUIRE(mp && o && out, SG_EINVAL, "null argument");
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative pair count");
  SG_REQUIRE(o->threshold_px > 0.0, SG_EINVAL, "threshold_px must be positive");
  SG_REQUIRE(o->max_hypotheses > 0, SG_EINVAL, "max_hypotheses must be positive");
  SG_REQUIRE(o->baseline >= 0.0, SG_EINVAL, "baseline must not be negative");
  SG_REQUIRE(n == 0 || pairs, SG_EINVAL, "null pair list");
  const sg_map& m = *mp;
  SG_REQUIRE(m.num_frames >= 0 && m.num_points >= 0 && m.num_obs >= 0 && m.num_cameras >= 0, SG_EINVAL,
             "negative map sizes");
  const int F = m.num_frames, P = m.num_points, M = m.num_obs;
  out->H = (std::min(o->max_hypotheses, kRelMaxHypotheses) + kRelThreads - 1) / kRelThreads * kRelThreads;
  out->S = out->H / kRelThreads;
  out->grid = (int64_t)n * out->S;
  SG_REQUIRE(out->grid <= 0x7fffffff, SG_EINVAL, "too many pairs for this many hypotheses");
  out->off.assign((size_t)n + 1, 0);
  out->records.clear();
  out->obs.clear();
  out->pairs.assign((size_t)n, RelPair{});
  out->num_run = 0;
  if (n == 0) return;
  std::vector<uint8_t> is_b((size_t)F, 0);
  for (int i = 0; i < n; ++i) {
    const int a = pairs[2 * i], b = pairs[2 * i + 1];
    SG_REQUIRE(a >= 0 && a < F && b >= 0 && b < F, SG_EINVAL, "frame index out of range");
    SG_REQUIRE(a != b, SG_EINVAL, "a pair of one frame");
    SG_REQUIRE(!is_b[b], SG_EINVAL, "the same b listed twice");
    is_b[b] = 1;
    const int ca = m.frame_camera[a], cb = m.frame_camera[b];
    SG_REQUIRE(m.k && ca >= 0 && ca < m.num_cameras && cb >= 0 && cb < m.num_cameras, SG_EINVAL,
               "the intrinsics of both frames cannot be read");
    RelPair& rp = out->pairs[i];
    std::memcpy(rp.ka, m.k + 7 * (size_t)ca, sizeof(rp.ka));
    std::memcpy(rp.kb, m.k + 7 * (size_t)cb, sizeof(rp.kb));
    rp.a = a;
    rp.b = b;
  }
  for (int ob = 0; ob < M; ++ob) {
    SG_REQUIRE(m.obs_frame[ob] >= 0 && m.obs_frame[ob] < F, SG_EINVAL, "obs_frame out of range");
    SG_REQUIRE(m.obs_point[ob] >= 0 && m.obs_point[ob] < P, SG_EINVAL, "obs_point out of range");
  }
  // per pair, two passes over the map's observations (they need not be grouped by frame): the first enabled
  // observation of each point in b, then a's enabled observations in map order, each point once
  std::vector<int32_t> first_b((size_t)P, -1), stamp_b((size_t)P, -1), seen_a((size_t)P, -1);
  for (int i = 0; i < n; ++i) {
    const int a = out->pairs[i].a, b = out->pairs[i].b;
    for (int ob = 0; ob < M; ++ob) {
      if (m.obs_frame[ob] != b || m.obs_disabled[ob] != 0) continue;
      const int p = m.obs_point[ob];
      if (stamp_b[p] == i) continue;
      stamp_b[p] = i;
      first_b[p] = ob;
    }
    for (int oa = 0; oa < M; ++oa) {
      if (m.obs_frame[oa] != a || m.obs_disabled[oa] != 0) continue;
      const int p = m.obs_point[oa];
      if (seen_a[p] == i) continue;
      seen_a[p] = i;
      if (stamp_b[p] != i) continue;
      const int ob = first_b[p];
      out->records.push_back(m.obs_pt[2 * (size_t)oa]);
      out->records.push_back(m.obs_pt[2 * (size_t)oa + 1]);
      out->records.push_back(m.obs_pt[2 * (size_t)ob]);
      out->records.push_back(m.obs_pt[2 * (size_t)ob + 1]);
      out->obs.push_back(oa);
      out->obs.push_back(ob);
    }
    SG_REQUIRE(out->obs.size() / 2 <= 0x7fffffff, SG_EINVAL, "too many records");
    out->off[i + 1] = (int32_t)(out->obs.size() / 2);
    out->pairs[i].run = out->off[i + 1] - out->off[i] >= kRelMinObs;
    out->num_run += out->pairs[i].run;
  }
}

}  // namespace sg
