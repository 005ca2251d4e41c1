// detect_math.h — the arithmetic of sg_tracker_detect (include/slamgpu.h), shared by the device kernel (detect.hip)
// and the CPU check (tests/native/detect_math_check.cpp), so that the two cannot drift apart: the ring of the
// radius-3 circle, the FAST-9 score from the 16 differences, the 3 x 3 suppression predicate, the ordered 64-bit key
// of (score, pixel index), the two-threshold eligibility, and the plain host functions: a level's cells as the
// kernel writes them (DetectLevelCells) and the compaction plus cap that turns cell slots into keypoints
// (DetectCompact).
//
// Every decision is an fp32 comparison, a min or a max of stored floats and of single differences of them: there is
// no sum and no product, so min / max may be taken in any grouping and the answer has no rounding freedom.
#ifndef SG_DETECT_MATH_H_
#define SG_DETECT_MATH_H_

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "slamgpu.h"

#if defined(__HIPCC__)
#define SG_DET_HD __host__ __device__ __forceinline__
#define SG_DET_UNROLL _Pragma("unroll")
#else
#define SG_DET_HD inline
#define SG_DET_UNROLL
#endif

namespace sg {

constexpr int kDetCell = 32;           // cells are 32 x 32 level pixels, anchored at pixel (0, 0)
constexpr int kDetRingRadius = 3;
constexpr int kDetMinBorder = 4, kDetMaxBorder = 64;
constexpr int kDetMaxPerCell = 16;
constexpr int kDetMaxCandidates = (kDetCell / 2) * (kDetCell / 2);   // one survivor per 2 x 2 block at most
constexpr int kDetMaxDepth = 8;        // kTrkMaxDepth

// The radius-3 Bresenham circle, clockwise from the top (image y pointing down).
struct DetRing {
  int8_t dx[16], dy[16];
};
static constexpr DetRing kDetRing = {{0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1},
                                     {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3}};

// max over the 16 arcs of the arc's smallest value: min over 9 = ((pairs of pairs) of pairs) and one more, which is
// the same value as any other grouping of the nine.
SG_DET_HD float DetectArcMax(const float* d) {
  float m2[16], m4[16];
SG_DET_UNROLL
  for (int k = 0; k < 16; ++k) m2[k] = fminf(d[k], d[(k + 1) & 15]);
SG_DET_UNROLL
  for (int k = 0; k < 16; ++k) m4[k] = fminf(m2[k], m2[(k + 2) & 15]);
  float best = fminf(fminf(m4[0], m4[4]), d[8]);
SG_DET_UNROLL
  for (int k = 1; k < 16; ++k) best = fmaxf(best, fminf(fminf(m4[k], m4[(k + 4) & 15]), d[(k + 8) & 15]));
  return best;
}

// s(p) from d_i = I(ring_i) - I(p): the largest threshold at which p is still a FAST-9 corner, bright or dark.
SG_DET_HD float DetectScore(const float* d) {
  float n[16];
SG_DET_UNROLL
  for (int k = 0; k < 16; ++k) n[k] = -d[k];
  return fmaxf(DetectArcMax(d), DetectArcMax(n));
}

// A cheap necessary condition of s(p) > t (t >= 0): every arc of nine holds two neighbouring compass pixels of the
// ring (0, 4, 8, 12), so two neighbouring compass differences must exceed t, or two must lie below -t.  Where it
// fails, s(p) <= t: the pixel is no candidate, and against a candidate (s > t_lo) it loses every comparison of the
// suppression exactly as t_lo itself would, so the kernel may store t_lo in its place.
SG_DET_HD bool DetectMayExceed(float d0, float d4, float d8, float d12, float t) {
  const bool b0 = d0 > t, b4 = d4 > t, b8 = d8 > t, b12 = d12 > t;
  const bool k0 = d0 < -t, k4 = d4 < -t, k8 = d8 < -t, k12 = d12 < -t;
  return (b0 && b4) || (b4 && b8) || (b8 && b12) || (b12 && b0) || (k0 && k4) || (k4 && k8) || (k8 && k12) ||
         (k12 && k0);
}

// 3 x 3 non-maximum suppression on a score array of row pitch `pitch`, c pointing at the pixel: strictly greater
// than the four neighbours earlier in row-major order, greater or equal to the four later ones.  Of two 8-adjacent
// pixels at most one survives.
SG_DET_HD bool DetectIsMax(const float* c, int pitch) {
  const float s = *c;
  return s > c[-pitch - 1] && s > c[-pitch] && s > c[-pitch + 1] && s > c[-1] && s >= c[1] && s >= c[pitch - 1] &&
         s >= c[pitch] && s >= c[pitch + 1];
}

SG_DET_HD bool DetectAdmissible(int x, int y, int w, int h, int border) {
  return x >= border && x <= w - 1 - border && y >= border && y <= h - 1 - border;
}

SG_DET_HD uint32_t DetectFloatBits(float s) {
  uint32_t b;
  __builtin_memcpy(&b, &s, 4);
  return b;
}

// (s, pixel index) as one ordered key, s > 0: a positive float's bits order like the float, and the index goes in
// complemented, so that a greater key is a greater score or, on a tie, a smaller index.  No candidate has key 0.
SG_DET_HD uint64_t DetectKey(float s, int index) { return ((uint64_t)DetectFloatBits(s) << 32) | (uint32_t)~(uint32_t)index; }
SG_DET_HD float DetectKeyScore(uint64_t key) {
  const uint32_t b = (uint32_t)(key >> 32);
  float s;
  __builtin_memcpy(&s, &b, 4);
  return s;
}
SG_DET_HD int DetectKeyIndex(uint64_t key) { return (int)~(uint32_t)key; }

// The two-threshold rule: with a candidate above t_hi in the cell only those are eligible, otherwise all are.
SG_DET_HD bool DetectEligible(uint64_t key, bool cell_has_high, float t_hi) {
  return key != 0 && (!cell_has_high || DetectKeyScore(key) > t_hi);
}

// -0.0f as a threshold means 0
SG_DET_HD float DetectThreshold(float t) { return t + 0.0f; }

inline int DetectCellsX(int w) { return (w + kDetCell - 1) / kDetCell; }
inline int DetectCells(int w, int h) { return DetectCellsX(w) * ((h + kDetCell - 1) / kDetCell); }

// What the kernel leaves per cell: per_cell key slots (the winners by descending key, then zeros) and two counts.
struct DetCellInfo {
  int32_t candidates, low;   // candidates before selection; 1 when the cell has candidates and none above t_hi
};

// One cell's selection, plainly: the eligible candidates by descending key, the first per_cell of them.
inline void DetectCellSelect(std::vector<uint64_t> cand, float t_hi, int per_cell, uint64_t* slots, DetCellInfo* info) {
  bool high = false;
  for (uint64_t k : cand) high = high || DetectKeyScore(k) > t_hi;
  info->candidates = (int32_t)cand.size();
  info->low = (!cand.empty() && !high) ? 1 : 0;
  std::vector<uint64_t> el;
  for (uint64_t k : cand)
    if (DetectEligible(k, high, t_hi)) el.push_back(k);
  std::sort(el.begin(), el.end(), [](uint64_t a, uint64_t b) { return a > b; });
  for (int r = 0; r < per_cell; ++r) slots[r] = r < (int)el.size() ? el[r] : 0;
}

// The contract on one packed w x h level, plainly: scores wherever a candidate or its neighbour can stand,
// suppression, the admissible test, and every cell's selection, in the layout the kernel writes
// (slots[cell * per_cell + rank], info[cell], cells row-major).
inline void DetectLevelCells(const float* img, int w, int h, float t_lo, float t_hi, int border, int per_cell,
                             uint64_t* slots, DetCellInfo* info) {
  const int cx = DetectCellsX(w), cells = DetectCells(w, h);
  std::vector<std::vector<uint64_t>> cand(cells);
  if (w > 2 * border && h > 2 * border) {
    const int x0 = border - 1, y0 = border - 1, sw = w - 2 * border + 2, sh = h - 2 * border + 2;
    std::vector<float> s((size_t)sw * sh);
    for (int y = 0; y < sh; ++y)
      for (int x = 0; x < sw; ++x) {
        const float* p = img + (size_t)(y0 + y) * w + (x0 + x);
        float d[16];
        for (int i = 0; i < 16; ++i) d[i] = p[kDetRing.dy[i] * w + kDetRing.dx[i]] - *p;
        s[(size_t)y * sw + x] = DetectScore(d);
      }
    for (int y = border; y <= h - 1 - border; ++y)
      for (int x = border; x <= w - 1 - border; ++x) {
        const float* c = &s[(size_t)(y - y0) * sw + (x - x0)];
        if (*c > t_lo && DetectIsMax(c, sw)) cand[(y / kDetCell) * cx + x / kDetCell].push_back(DetectKey(*c, y * w + x));
      }
  }
  for (int c = 0; c < cells; ++c) DetectCellSelect(cand[c], t_hi, per_cell, slots + (size_t)c * per_cell, info + c);
}

// One level of a detect call, as DetectCompact reads it: its number, its size, and where its cells start.
struct DetLevel {
  int level, w, h, cell0, cells;
};

struct DetKeypoint {
  float x, y, score;   // level-0 pixels
  int32_t level;
};

// Host-side compaction plus cap.  From the cell slots of the selected levels (ascending), the keypoints in the
// order level, cell row-major, rank within the cell; with max_keypoints > 0 and more keypoints than that, only the
// max_keypoints best by (score descending, level ascending, pixel index ascending) stay, in the same order.
// per_level (may be null) has `depth` records whose sizes the caller has filled: the selected ones get cells,
// candidates, low_cells and keypoints.
inline std::vector<DetKeypoint> DetectCompact(const std::vector<DetLevel>& lv, const uint64_t* slots,
                                              const DetCellInfo* info, int per_cell, int max_keypoints,
                                              sg_detect_level* per_level) {
  struct Item {
    uint64_t key;
    int li;
  };
  std::vector<Item> all;
  for (int li = 0; li < (int)lv.size(); ++li)
    for (int c = 0; c < lv[li].cells; ++c)
      for (int r = 0; r < per_cell; ++r) {
        const uint64_t k = slots[(size_t)(lv[li].cell0 + c) * per_cell + r];
        if (k == 0) break;
        all.push_back({k, li});
      }
  std::vector<char> keep(all.size(), 1);
  if (max_keypoints > 0 && (size_t)max_keypoints < all.size()) {
    std::vector<int> order(all.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    auto better = [&](int a, int b) {   // score descending, level ascending, pixel index ascending
      const uint32_t sa = (uint32_t)(all[a].key >> 32), sb = (uint32_t)(all[b].key >> 32);
      if (sa != sb) return sa > sb;
      if (all[a].li != all[b].li) return all[a].li < all[b].li;
      return (uint32_t)all[a].key > (uint32_t)all[b].key;   // the complemented index
    };
    std::nth_element(order.begin(), order.begin() + max_keypoints, order.end(), better);
    std::fill(keep.begin(), keep.end(), 0);
    for (int i = 0; i < max_keypoints; ++i) keep[order[i]] = 1;
  }
  if (per_level)
    for (const DetLevel& l : lv) {
      sg_detect_level& r = per_level[l.level];
      r.cells = l.cells;
      r.candidates = r.low_cells = r.keypoints = 0;
      for (int c = 0; c < l.cells; ++c) {
        r.candidates += info[l.cell0 + c].candidates;
        r.low_cells += info[l.cell0 + c].low;
      }
    }
  std::vector<DetKeypoint> out;
  for (size_t i = 0; i < all.size(); ++i) {
    if (!keep[i]) continue;
    const DetLevel& l = lv[all[i].li];
    const int idx = DetectKeyIndex(all[i].key), x = idx % l.w, y = idx / l.w;
    const float scale = (float)(1 << l.level);
    out.push_back({(float)x * scale, (float)y * scale, DetectKeyScore(all[i].key), (int32_t)l.level});
    if (per_level) ++per_level[l.level].keypoints;
  }
  return out;
}

}  // namespace sg

#endif  // SG_DETECT_MATH_H_
