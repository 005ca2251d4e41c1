// detect.hip — sg_tracker_detect: FAST-9 corners on the blurred float pyramid a tracker slot already holds, spread
// over the image by 32 x 32 cells.  The arithmetic is detect_math.h's, shared with the CPU check.
//
//   k_detect  one workgroup of 256 threads per cell, the cells of all selected levels in one launch (a by-value level
//             table with a cell prefix maps blockIdx to level and cell).  The workgroup stages the cell and a 4-pixel
//             halo in LDS (40 x 40 floats, pitch 41, loads clamped to the level), computes the score on the 34 x 34
//             block that holds the cell and its one-pixel ring from LDS (a four-compass-pixel reject first), and then
//             each thread owns one 2 x 2 block of the cell: of its four pixels at most one survives the suppression,
//             so its key has a fixed LDS slot and no compaction order exists.  A workgroup OR decides the
//             two-threshold branch, each eligible key is ranked by counting the greater keys (LDS broadcasts), and the
//             per_cell winners go to the cell's own slots in global memory with the cell's candidate count and branch.
//             No atomics; LDS 6560 + 4760 + 2048 bytes.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "detect_math.h"
#include "tracker.h"

namespace sg {

namespace {

constexpr int kDetThreads = 256;
constexpr int kDetHalo = 4;                              // ring radius 3 + the suppression's one pixel
constexpr int kDetTile = kDetCell + 2 * kDetHalo;        // 40
constexpr int kDetTilePitch = kDetTile + 1;              // odd: a column of the tile spreads over the banks
constexpr int kDetScore = kDetCell + 2;                  // 34: the cell and its one-pixel ring
constexpr int kDetScorePitch = kDetScore + 1;
static_assert(kDetMaxCandidates == kDetThreads, "one 2 x 2 block of the cell per thread");
static_assert(kDetMaxDepth == kTrkMaxDepth, "the level table holds every level of a tracker");
static_assert(kDetHalo == kDetRingRadius + 1 && kDetHalo <= kDetMinBorder, "the halo covers ring and suppression");

struct DetPyr {
  const float* img[kTrkMaxDepth];           // entry i: the i-th selected level
  int w[kTrkMaxDepth], h[kTrkMaxDepth];
  int cell0[kTrkMaxDepth + 1];              // cell prefix: cells of entry i are cell0[i] .. cell0[i + 1] - 1
  int n;
};

__global__ __launch_bounds__(kDetThreads) void k_detect(DetPyr pyr, float t_lo, float t_hi, int border, int per_cell,
                                                        uint64_t* __restrict__ slots,
                                                        DetCellInfo* __restrict__ info) {
  __shared__ float tile[kDetTile * kDetTilePitch];
  __shared__ float sc[kDetScore * kDetScorePitch];
  __shared__ uint64_t keys[kDetThreads];
  const int tid = threadIdx.x, cell = blockIdx.x;   // cell < cell0[n]: the grid is exactly the cells
  int li = 0;
  while (li + 1 < pyr.n && cell >= pyr.cell0[li + 1]) ++li;   // workgroup-uniform
  const float* __restrict__ img = pyr.img[li];
  const int w = pyr.w[li], h = pyr.h[li];
  const int c = cell - pyr.cell0[li], cells_x = (w + kDetCell - 1) / kDetCell;
  const int x0 = (c % cells_x) * kDetCell, y0 = (c / cells_x) * kDetCell;

  // the cell and its halo; coordinates clamped to the level, so every load is inside it
  for (int i = tid; i < kDetTile * kDetTile; i += kDetThreads) {
    const int ty = i / kDetTile, tx = i - ty * kDetTile;
    const int gx = min(max(x0 - kDetHalo + tx, 0), w - 1), gy = min(max(y0 - kDetHalo + ty, 0), h - 1);
    tile[ty * kDetTilePitch + tx] = img[(size_t)gy * w + gx];
  }
  __syncthreads();

  // scores of the cell and its one-pixel ring.  A pixel whose ring leaves the level gets a value of clamped loads:
  // it is inadmissible and so are all its neighbours (border >= 4), so nothing reads it.
  for (int i = tid; i < kDetScore * kDetScore; i += kDetThreads) {
    const int sy = i / kDetScore, sx = i - sy * kDetScore;
    const float* p = tile + (sy + kDetHalo - 1) * kDetTilePitch + (sx + kDetHalo - 1);
    const float v = *p;
    const float d0 = p[-3 * kDetTilePitch] - v, d4 = p[3] - v, d8 = p[3 * kDetTilePitch] - v, d12 = p[-3] - v;
    float s = t_lo;   // DetectMayExceed: stands for any score <= t_lo
    if (DetectMayExceed(d0, d4, d8, d12, t_lo)) {
      float d[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) d[k] = p[kDetRing.dy[k] * kDetTilePitch + kDetRing.dx[k]] - v;
      s = DetectScore(d);
    }
    sc[sy * kDetScorePitch + sx] = s;
  }
  __syncthreads();

  // this thread's 2 x 2 block: at most one of its pixels survives
  const int bx = 2 * (tid & 15), by = 2 * (tid >> 4);
  uint64_t key = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int lx = bx + (q & 1), ly = by + (q >> 1), x = x0 + lx, y = y0 + ly;
    const float* cs = sc + (ly + 1) * kDetScorePitch + (lx + 1);
    if (DetectAdmissible(x, y, w, h, border) && *cs > t_lo && DetectIsMax(cs, kDetScorePitch)) key = DetectKey(*cs, y * w + x);
  }
  const int candidates = __syncthreads_count(key != 0);
  if (candidates == 0) {   // workgroup-uniform
    if (tid < per_cell) slots[(size_t)cell * per_cell + tid] = 0;
    if (tid == 0) info[cell] = DetCellInfo{0, 0};
    return;
  }
  const bool high = __syncthreads_or(key != 0 && DetectKeyScore(key) > t_hi) != 0;
  const uint64_t mine = DetectEligible(key, high, t_hi) ? key : 0;
  keys[tid] = mine;
  const int eligible = __syncthreads_count(mine != 0);   // and the barrier that publishes keys[]

  int rank = 0;
  for (int j = 0; j < kDetThreads; ++j) rank += keys[j] > mine ? 1 : 0;   // keys of one level are distinct
  if (mine != 0 && rank < per_cell) slots[(size_t)cell * per_cell + rank] = mine;
  if (tid < per_cell && tid >= eligible) slots[(size_t)cell * per_cell + tid] = 0;
  if (tid == 0) info[cell] = DetCellInfo{candidates, high ? 0 : 1};
}

}  // namespace

void Tracker::Detect(int slot, const sg_detect_options& o, int cap, float* xy, int32_t* levels, float* score,
                     int32_t* count, sg_detect_level* per_level) {
  // every refusal before the device is touched, with nothing written
  SG_REQUIRE(count, SG_EINVAL, "null count");
  SG_REQUIRE(cap >= 0 && (cap == 0 || (xy && levels)), SG_EINVAL, "bad capacity or null keypoint arrays");
  SG_REQUIRE(slot >= 0 && slot < (int)slots_.size() && slots_[slot].valid, SG_EINVAL, "empty slot");
  SG_REQUIRE(o.first_level >= 0 && o.first_level < opt_.depth, SG_EINVAL, "first_level outside the pyramid");
  SG_REQUIRE(o.num_levels >= 0 && o.num_levels <= opt_.depth - o.first_level, SG_EINVAL,
             "level range runs past the pyramid");
  SG_REQUIRE(std::isfinite(o.threshold) && std::isfinite(o.min_threshold) && o.min_threshold >= 0.f &&
                 o.min_threshold <= o.threshold,
             SG_EINVAL, "thresholds must be finite with 0 <= min_threshold <= threshold");
  SG_REQUIRE(o.border >= kDetMinBorder && o.border <= kDetMaxBorder, SG_EINVAL, "border must be 4..64");
  SG_REQUIRE(o.per_cell >= 1 && o.per_cell <= kDetMaxPerCell, SG_EINVAL, "per_cell must be 1..16");
  SG_REQUIRE(o.max_keypoints >= 0, SG_EINVAL, "negative max_keypoints");
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  const Slot& s = slots_[slot];
  const int nl = o.num_levels ? o.num_levels : opt_.depth - o.first_level;
  const float t_lo = DetectThreshold(o.min_threshold), t_hi = DetectThreshold(o.threshold);
  DetPyr pyr{};
  std::vector<DetLevel> lv(nl);
  int cells = 0;
  for (int i = 0; i < nl; ++i) {
    const int l = o.first_level + i;
    pyr.img[i] = s.pyr.ptr + s.off[l];
    pyr.w[i] = s.w[l];
    pyr.h[i] = s.h[l];
    pyr.cell0[i] = cells;
    lv[i] = DetLevel{l, s.w[l], s.h[l], cells, DetectCells(s.w[l], s.h[l])};
    cells += lv[i].cells;
  }
  pyr.cell0[nl] = cells;
  pyr.n = nl;
  det_slots_.Resize((size_t)cells * o.per_cell);
  det_info_.Resize(cells);
  det_slots_h_.resize((size_t)cells * o.per_cell);
  det_info_h_.resize(cells);
  SG_HIP_CHECK(hipEventRecord(ev_[6], stream_));
  hipLaunchKernelGGL(k_detect, dim3(cells), dim3(kDetThreads), 0, stream_, pyr, t_lo, t_hi, o.border, o.per_cell,
                     det_slots_.ptr, det_info_.ptr);
  SG_HIP_CHECK(hipEventRecord(ev_[7], stream_));
  SG_HIP_CHECK(hipGetLastError());
  SG_HIP_CHECK(hipMemcpyAsync(det_slots_h_.data(), det_slots_.ptr, sizeof(uint64_t) * det_slots_h_.size(),
                              hipMemcpyDeviceToHost, stream_));
  SG_HIP_CHECK(hipMemcpyAsync(det_info_h_.data(), det_info_.ptr, sizeof(DetCellInfo) * cells, hipMemcpyDeviceToHost,
                              stream_));
  SG_HIP_CHECK(hipStreamSynchronize(stream_));
  float ms = 0.f;
  SG_HIP_CHECK(hipEventElapsedTime(&ms, ev_[6], ev_[7]));
  detect_ms_ = ms;

  if (per_level)
    for (int l = 0; l < opt_.depth; ++l) per_level[l] = sg_detect_level{s.w[l], s.h[l], 0, 0, 0, 0};
  const std::vector<DetKeypoint> kp =
      DetectCompact(lv, det_slots_h_.data(), det_info_h_.data(), o.per_cell, o.max_keypoints, per_level);
  *count = (int32_t)kp.size();
  const int n = std::min<int>(cap, (int)kp.size());
  for (int i = 0; i < n; ++i) {
    xy[2 * i] = kp[i].x;
    xy[2 * i + 1] = kp[i].y;
    levels[i] = kp[i].level;
    if (score) score[i] = kp[i].score;
  }
}

}  // namespace sg
