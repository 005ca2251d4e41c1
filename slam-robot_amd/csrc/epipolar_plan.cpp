// epipolar_plan.cpp — see epipolar_plan.h.
#include "epipolar_plan.h"

#include <algorithm>
#include <cmath>

#include "common.h"
#include "match_plan.h"

namespace sg {

namespace {

void CheckSide(const int32_t* offset, int32_t n, const double* xy, const uint64_t* desc, const int32_t* level) {
  SG_REQUIRE(offset[0] == 0, SG_EINVAL, "a keypoint offset array must start at 0");
  for (int i = 0; i < n; ++i) SG_REQUIRE(offset[i + 1] >= offset[i], SG_EINVAL, "decreasing keypoint offset");
  const int32_t K = offset[n];
  SG_REQUIRE(K <= kEpiMaxKeypoints, SG_EINVAL, "more than 2^20 keypoints on one side in one call");
  SG_REQUIRE(K == 0 || (xy && desc), SG_EINVAL, "null keypoints");
  if (level)
    for (int32_t k = 0; k < K; ++k)
      SG_REQUIRE(level[k] >= 0 && level[k] <= kEpiMaxLevel, SG_EINVAL, "keypoint level outside 0..7");
}

}  // namespace

void PlanEpipolar(const sg_map* mp, const int32_t* pairs, int32_t n, const int32_t* a_offset, const double* a_xy,
                  const uint64_t* a_desc, const int32_t* a_level, const int32_t* b_offset, const double* b_xy,
                  const uint64_t* b_desc, const int32_t* b_level, const sg_epipolar_options* o, EpipolarPlan* out) {
  SG_REQUIRE(mp && o && out, SG_EINVAL, "null argument");
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative count");
  SG_REQUIRE(o->tol_px > 0.0 && std::isfinite(o->tol_px), SG_EINVAL, "tol_px must be positive and finite");
  SG_REQUIRE(o->min_parallax >= 0.0 && std::isfinite(o->min_parallax), SG_EINVAL,
             "min_parallax must be finite and not negative");
  SG_REQUIRE(o->max_dist >= 0 && o->max_dist <= 256, SG_EINVAL, "max_dist must be in 0..256");
  SG_REQUIRE(o->ratio_percent >= 1 && o->ratio_percent <= 100, SG_EINVAL, "ratio_percent must be in 1..100");
  *out = EpipolarPlan{};
  out->n = n;
  if (n == 0) return;
  const sg_map& m = *mp;
  SG_REQUIRE(pairs && a_offset && b_offset, SG_EINVAL, "null pair list or keypoint offsets");
  SG_REQUIRE((a_level == nullptr) == (b_level == nullptr), SG_EINVAL, "levels on one side only");
  CheckSide(a_offset, n, a_xy, a_desc, a_level);
  CheckSide(b_offset, n, b_xy, b_desc, b_level);
  SG_REQUIRE(m.num_frames >= 0 && m.num_cameras >= 0, SG_EINVAL, "negative map sizes");
  SG_REQUIRE(m.q && m.t && m.k && m.frame_camera, SG_EINVAL, "the map's poses or cameras cannot be read");
  int64_t cap = 0;
  for (int i = 0; i < n; ++i) {
    const int fa = pairs[2 * i], fb = pairs[2 * i + 1];
    SG_REQUIRE(fa >= 0 && fa < m.num_frames && fb >= 0 && fb < m.num_frames, SG_EINVAL, "frame index out of range");
    SG_REQUIRE(fa != fb, SG_EINVAL, "a pair of one frame with itself");
    for (int f : {fa, fb})
      SG_REQUIRE(m.frame_camera[f] >= 0 && m.frame_camera[f] < m.num_cameras, SG_EINVAL, "camera index out of range");
    const int64_t na = a_offset[i + 1] - a_offset[i], nb = b_offset[i + 1] - b_offset[i];
    cap += na * ((nb + kEpiSlice - 1) / kEpiSlice);
  }
  SG_REQUIRE(cap <= kEpiMaxPartials, SG_EINVAL, "partial results above 128 MiB: split the pairs over calls");

  out->KA = a_offset[n];
  out->KB = b_offset[n];
  out->levels = a_level != nullptr;
  out->pairs.resize((size_t)n);
  out->live.assign((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    const int fa = pairs[2 * i], fb = pairs[2 * i + 1];
    EpiPair& p = out->pairs[i];
    EpiPairFrom(m.q + 4 * (size_t)fa, m.t + 3 * (size_t)fa, m.k + 7 * (size_t)m.frame_camera[fa], m.q + 4 * (size_t)fb,
                m.t + 3 * (size_t)fb, m.k + 7 * (size_t)m.frame_camera[fb], &p);
    const int32_t na = a_offset[i + 1] - a_offset[i], nb = b_offset[i + 1] - b_offset[i];
    if (p.degenerate || na == 0 || nb == 0) continue;
    out->live[i] = 1;
    for (int32_t k0 = a_offset[i]; k0 < a_offset[i + 1]; k0 += kEpiPrepRun)
      out->prep.push_back(EpiPrepItem{i, 0, k0, std::min<int32_t>(kEpiPrepRun, a_offset[i + 1] - k0)});
    for (int32_t k0 = b_offset[i]; k0 < b_offset[i + 1]; k0 += kEpiPrepRun)
      out->prep.push_back(EpiPrepItem{i, 1, k0, std::min<int32_t>(kEpiPrepRun, b_offset[i + 1] - k0)});
    const int32_t slices = (nb + kEpiSlice - 1) / kEpiSlice;
    const int32_t base = (int32_t)out->partials;   // (<= 2^23)
    for (int32_t c0 = 0; c0 < na; c0 += kEpiChunk) {
      const int32_t cc = std::min<int32_t>(kEpiChunk, na - c0);
      out->chunks.push_back(EpiChunkItem{a_offset[i] + c0, cc, base + c0, na, slices, {0, 0, 0}});
      for (int32_t s = 0; s < slices; ++s) {
        const int32_t j0 = s * kEpiSlice;
        out->items.push_back(EpiItem{i, a_offset[i] + c0, cc, b_offset[i] + j0, std::min<int32_t>(kEpiSlice, nb - j0),
                                     j0, base + s * na + c0, 0});
      }
    }
    out->partials += (int64_t)na * slices;
  }
  out->launch = !out->items.empty();
}

void ResolveEpipolar(const EpipolarPlan& plan, const int32_t* a_offset, const int32_t* b_offset, const int32_t* best_kp,
                     const int32_t* best_dist, const int32_t* second_dist, const int32_t* num_candidates,
                     const sg_epipolar_options& o, int32_t* match, sg_epipolar_result* results) {
  sg_match_options mo{};
  mo.max_dist = o.max_dist;
  mo.ratio_percent = o.ratio_percent;
  std::vector<sg_match_result> mr((size_t)plan.n, sg_match_result{});
  ResolveMatches(a_offset, plan.n, best_kp, best_dist, second_dist, num_candidates, mo, match, mr.data());
  if (!results) return;
  for (int i = 0; i < plan.n; ++i) {
    results[i].num_a = a_offset[i + 1] - a_offset[i];
    results[i].num_b = b_offset[i + 1] - b_offset[i];
    results[i].num_with_candidates = mr[i].num_with_candidates;
    results[i].num_matched = mr[i].num_matched;
    results[i].degenerate = plan.pairs[i].degenerate;
  }
}

void RunEpipolarCpu(const EpipolarPlan& plan, const int32_t* a_offset, const double* a_xy, const uint64_t* a_desc,
                    const int32_t* a_level, const int32_t* b_offset, const double* b_xy, const uint64_t* b_desc,
                    const int32_t* b_level, const sg_epipolar_options& o, int32_t* best_kp, int32_t* best_dist,
                    int32_t* second_dist, int32_t* num_candidates) {
  const double tol2 = o.tol_px * o.tol_px;
  std::vector<EpiB> brec;
  for (int i = 0; i < plan.n; ++i) {
    for (int32_t k = a_offset[i]; k < a_offset[i + 1]; ++k) {
      best_kp[k] = best_dist[k] = second_dist[k] = -1;
      num_candidates[k] = 0;
    }
    if (!plan.live[i]) continue;
    const EpiPair& p = plan.pairs[i];
    const int32_t nb = b_offset[i + 1] - b_offset[i];
    brec.resize((size_t)nb);
    for (int32_t j = 0; j < nb; ++j) {
      const size_t kb = (size_t)b_offset[i] + j;
      EpiPrepB(p, b_xy + 2 * kb, b_level ? b_level[kb] : 0, &brec[j]);
    }
    for (int32_t k = a_offset[i]; k < a_offset[i + 1]; ++k) {
      EpiA a;
      EpiPrepA(p, a_xy + 2 * (size_t)k, a_level ? a_level[k] : 0, &a);
      const uint64_t* da = a_desc + 4 * (size_t)k;
      int d1 = -1, d2 = -1, j1 = -1, count = 0;   // smallest and second smallest distance; ties keep the earlier j
      for (int32_t j = 0; j < nb; ++j) {
        if (!EpiCandidate(a, brec[j], tol2, o.min_parallax)) continue;
        const uint64_t* db = b_desc + 4 * ((size_t)b_offset[i] + j);
        int h = 0;
        for (int w = 0; w < 4; ++w) h += __builtin_popcountll(da[w] ^ db[w]);
        ++count;
        if (d1 < 0 || h < d1) {
          d2 = d1;
          d1 = h;
          j1 = j;
        } else if (d2 < 0 || h < d2) {
          d2 = h;
        }
      }
      best_kp[k] = j1;
      best_dist[k] = d1;
      second_dist[k] = d2;
      num_candidates[k] = count;
    }
  }
}

}  // namespace sg
