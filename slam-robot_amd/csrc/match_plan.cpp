// match_plan.cpp — see match_plan.h.
#include "match_plan.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"

namespace sg {

void PlanMatch(const sg_map* mp, const int32_t* frames, int32_t n, const int32_t* kp_offset, const double* kp_xy,
               const uint64_t* kp_desc, const int32_t* points, int32_t np, const uint64_t* point_desc,
               const sg_match_options* o, MatchPlan* out) {
  SG_REQUIRE(mp && o && out, SG_EINVAL, "null argument");
  SG_REQUIRE(n >= 0 && np >= 0, SG_EINVAL, "negative count");
  SG_REQUIRE(o->radius_px > 0.0 && std::isfinite(o->radius_px), SG_EINVAL, "radius_px must be positive and finite");
  SG_REQUIRE(o->width >= 0 && o->height >= 0 && (o->width == 0) == (o->height == 0), SG_EINVAL,
             "width and height must be both positive or both zero");
  SG_REQUIRE(o->max_dist >= 0 && o->max_dist <= 256, SG_EINVAL, "max_dist must be in 0..256");
  SG_REQUIRE(o->ratio_percent >= 1 && o->ratio_percent <= 100, SG_EINVAL, "ratio_percent must be in 1..100");
  *out = MatchPlan{};
  out->n = n;
  out->np = np;
  if (n == 0) return;
  const sg_map& m = *mp;
  SG_REQUIRE(frames && kp_offset, SG_EINVAL, "null frame list or keypoint offsets");
  SG_REQUIRE(kp_offset[0] == 0, SG_EINVAL, "kp_offset[0] must be 0");
  for (int i = 0; i < n; ++i) SG_REQUIRE(kp_offset[i + 1] >= kp_offset[i], SG_EINVAL, "decreasing keypoint offset");
  const int32_t K = kp_offset[n];
  SG_REQUIRE(K <= kMatchMaxKeypoints, SG_EINVAL, "more than 2^20 keypoints in one call");
  SG_REQUIRE(K == 0 || (kp_xy && kp_desc), SG_EINVAL, "null keypoints");
  SG_REQUIRE(np == 0 || (points && point_desc), SG_EINVAL, "null point list or descriptors");
  SG_REQUIRE((int64_t)n * np <= kMatchMaxPairs, SG_EINVAL, "n * np is above 2^22: split the frames over calls");
  SG_REQUIRE(m.num_frames >= 0 && m.num_points >= 0 && m.num_cameras >= 0 && m.num_obs >= 0, SG_EINVAL,
             "negative map sizes");
  SG_REQUIRE(m.q && m.t && m.k && m.frame_camera, SG_EINVAL, "the map's poses or cameras cannot be read");
  SG_REQUIRE(np == 0 || m.X, SG_EINVAL, "the map's points cannot be read");
  for (int i = 0; i < n; ++i) {
    const int f = frames[i];
    SG_REQUIRE(f >= 0 && f < m.num_frames, SG_EINVAL, "frame index out of range");
    SG_REQUIRE(m.frame_camera[f] >= 0 && m.frame_camera[f] < m.num_cameras, SG_EINVAL, "camera index out of range");
  }
  std::vector<int32_t> pos_of((size_t)m.num_points, -1);   // the point's position in points[], -1: not listed
  for (int j = 0; j < np; ++j) {
    const int p = points[j];
    SG_REQUIRE(p >= 0 && p < m.num_points, SG_EINVAL, "point index out of range");
    SG_REQUIRE(pos_of[p] < 0, SG_EINVAL, "a point listed twice");
    pos_of[p] = j;
  }
  const bool skip = o->skip_observed != 0;
  if (skip && m.num_obs > 0) {
    SG_REQUIRE(m.obs_frame && m.obs_point && m.obs_disabled, SG_EINVAL, "the map's observations cannot be read");
    for (int32_t ob = 0; ob < m.num_obs; ++ob)
      SG_REQUIRE(m.obs_frame[ob] >= 0 && m.obs_frame[ob] < m.num_frames && m.obs_point[ob] >= 0 &&
                     m.obs_point[ob] < m.num_points,
                 SG_EINVAL, "observation index out of range");
  }

  out->K = K;
  out->words = (np + 31) / 32;
  out->slices = (np + kMatchSlice - 1) / kMatchSlice;
  out->project_blocks = (np + 255) / 256;
  out->launch = K > 0 && np > 0;
  out->frames.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int f = frames[i];
    MatchFrame& mf = out->frames[i];
    std::memcpy(mf.q, m.q + 4 * (size_t)f, sizeof(mf.q));
    std::memcpy(mf.t, m.t + 3 * (size_t)f, sizeof(mf.t));
    std::memcpy(mf.k, m.k + 7 * (size_t)m.frame_camera[f], sizeof(mf.k));
  }
  out->X.resize(4 * (size_t)np);
  for (int j = 0; j < np; ++j) std::memcpy(&out->X[4 * (size_t)j], m.X + 4 * (size_t)points[j], 4 * sizeof(double));
  out->excl.assign((size_t)n * out->words, 0u);
  if (skip && np > 0 && m.num_obs > 0) {
    // the listed slots of each map frame, chained: head[f] -> next[slot] -> ... (a frame may be listed more than once)
    std::vector<int32_t> head((size_t)m.num_frames, -1), next((size_t)n, -1);
    for (int i = n - 1; i >= 0; --i) {
      next[i] = head[frames[i]];
      head[frames[i]] = i;
    }
    for (int32_t ob = 0; ob < m.num_obs; ++ob) {
      if (m.obs_disabled[ob] != 0) continue;
      const int j = pos_of[m.obs_point[ob]];
      if (j < 0) continue;
      for (int i = head[m.obs_frame[ob]]; i >= 0; i = next[i])
        out->excl[(size_t)i * out->words + (j >> 5)] |= 1u << (j & 31);
    }
  }
  for (int i = 0; i < n; ++i)
    for (int32_t k0 = kp_offset[i]; k0 < kp_offset[i + 1]; k0 += kMatchChunk)
      out->chunks.push_back(MatchChunk{i, k0, std::min<int32_t>(kMatchChunk, kp_offset[i + 1] - k0), 0});
}

void ResolveMatches(const int32_t* kp_offset, int32_t n, const int32_t* best_point, const int32_t* best_dist,
                    const int32_t* second_dist, const int32_t* num_candidates, const sg_match_options& o,
                    int32_t* match, sg_match_result* results) {
  struct Claim {
    int32_t point, dist, kp;
  };
  std::vector<Claim> claims;
  for (int i = 0; i < n; ++i) {
    claims.clear();
    int with = 0;
    for (int32_t k = kp_offset[i]; k < kp_offset[i + 1]; ++k) {
      match[k] = -1;
      with += num_candidates[k] > 0;
      if (best_point[k] < 0 || best_dist[k] > o.max_dist) continue;
      if (second_dist[k] >= 0 && 100 * best_dist[k] > o.ratio_percent * second_dist[k]) continue;
      claims.push_back(Claim{best_point[k], best_dist[k], k});
    }
    std::sort(claims.begin(), claims.end(), [](const Claim& a, const Claim& b) {
      if (a.point != b.point) return a.point < b.point;
      if (a.dist != b.dist) return a.dist < b.dist;
      return a.kp < b.kp;
    });
    int matched = 0;
    for (size_t c = 0; c < claims.size(); ++c) {
      if (c > 0 && claims[c].point == claims[c - 1].point) continue;   // a later claimant of the same point
      match[claims[c].kp] = claims[c].point;
      ++matched;
    }
    if (results) {
      results[i].num_with_candidates = with;
      results[i].num_matched = matched;
    }
  }
}

}  // namespace sg
