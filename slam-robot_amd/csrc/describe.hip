// describe.hip — sg_tracker_describe: oriented 256-bit descriptors (steered BRIEF) of keypoints on the blurred
// float pyramid a tracker slot already holds.  The arithmetic is describe_math.h's, shared with the CPU check.
//
//   k_describe  one wavefront per keypoint, four per workgroup, one launch per call for keypoints on any levels.
//               The wave copies the 31 x 31 patch around the keypoint's centre pixel into its own LDS region
//               (row pitch 31: an odd pitch, so a column of the patch spreads over the banks); lane l adds the
//               disc pixels l, l + 64, ... of the two first moments in fp64 from LDS and wave_sum_full's fixed
//               tree gives every lane both sums, and so the bin; four rounds of one pattern row per lane, two LDS
//               pixels and a ballot give the four descriptor words.  No bit is assembled in memory, no atomic is
//               used, and the kernel has no workgroup barrier: a wave past n or a refused keypoint just leaves,
//               and a wave touches no LDS but its own region.
#include <hip/hip_runtime.h>

#include "ba_device.h"
#include "common.h"
#include "describe_math.h"
#include "tracker.h"

namespace sg {

namespace {

constexpr int kDescWaves = 4;                                  // keypoints per workgroup (one wave each)
constexpr int kDescPatchLen = kDescPatch * kDescPatch;         // 961 floats, 3844 bytes per wave
constexpr int kDescCopy = (kDescPatchLen + 63) / 64;           // patch values per lane: 16 (lane 0), else 15
static_assert(kDescLanes == 64, "one disc partial per lane of a wave");
static_assert(kDescOk == SG_DESC_OK && kDescBorder == SG_DESC_BORDER, "describe_math.h's statuses are the header's");

struct DescPyr {
  const float* img[kTrkMaxDepth];
  int w[kTrkMaxDepth], h[kTrkMaxDepth];
};

__global__ __launch_bounds__(64 * kDescWaves) void k_describe(DescPyr pyr, int n, const float* __restrict__ xy,
                                                              const int32_t* __restrict__ levels,
                                                              uint64_t* __restrict__ desc,
                                                              int32_t* __restrict__ angle_bin,
                                                              int32_t* __restrict__ status) {
  __shared__ float patches[kDescWaves][kDescPatchLen];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * kDescWaves + wave;
  if (f >= n) return;   // whole wave (no workgroup barrier below)
  const int lv = __builtin_amdgcn_readfirstlane(levels[f]);   // 0 .. depth - 1: checked on the host
  const int w = pyr.w[lv], h = pyr.h[lv];
  int cx, cy;
  if (!DescCentre(xy[2 * f], xy[2 * f + 1], lv, w, h, &cx, &cy)) {   // wave-uniform
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) desc[4 * (size_t)f + r] = 0;
      angle_bin[f] = -1;
      status[f] = kDescBorder;
    }
    return;
  }

  // the patch: rows cy - 15 .. cy + 15, columns cx - 15 .. cx + 15, all inside the level (DescCentre)
  float* P = patches[wave];
  const float* src = pyr.img[lv] + (size_t)(cy - kDescRadius) * w + (cx - kDescRadius);
  float pv[kDescCopy];
#pragma unroll
  for (int k = 0; k < kDescCopy; ++k) {
    const int idx = min(lane + 64 * k, kDescPatchLen - 1), r = idx / kDescPatch;
    pv[k] = src[(size_t)r * w + (idx - r * kDescPatch)];   // unconditional: the loads are in flight together
  }
#pragma unroll
  for (int k = 0; k < kDescCopy; ++k) {
    const int idx = lane + 64 * k;
    if (idx < kDescPatchLen) P[idx] = pv[k];
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const float* C = P + kDescRadius * kDescPatch + kDescRadius;   // the centre pixel

  // first moments of the disc, describe_math.h's order: this lane's 12 pixels in turn, then the lane tree
  double a = 0.0, b = 0.0;
#pragma unroll
  for (int k = 0; k < kDescPerLane; ++k) {
    const int i = lane + kDescLanes * k, u = kDescDisc.u[i], v = kDescDisc.v[i];
    const float I = C[v * kDescPatch + u];
    a = DescAcc(a, u, I);
    b = DescAcc(b, v, I);
  }
  const double m10 = wave_sum_full(a), m01 = wave_sum_full(b);
  const int bin = __builtin_amdgcn_readfirstlane(DescBin(m10, m01));   // the same in every lane

  // test 64 r + lane: one 32-bit pattern row (ax, ay, bx, by), two LDS pixels, bit `lane` of word r by ballot
  unsigned long long word[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    uint32_t t;
    __builtin_memcpy(&t, kBriefPattern[bin][64 * r + lane], 4);
    const int ax = (int8_t)(t & 0xFF), ay = (int8_t)((t >> 8) & 0xFF);
    const int bx = (int8_t)((t >> 16) & 0xFF), by = (int8_t)(t >> 24);
    const float pa = C[ay * kDescPatch + ax], pb = C[by * kDescPatch + bx];
    word[r] = __ballot(pa < pb);
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) desc[4 * (size_t)f + r] = word[r];
    angle_bin[f] = bin;
    status[f] = kDescOk;
  }
}

}  // namespace

void Tracker::Describe(int slot, int n, const float* xy, const int32_t* levels, uint64_t* desc, int32_t* angle_bin,
                       int32_t* status) {
  // every refusal before the device is touched, with nothing written
  SG_REQUIRE(n >= 0 && n <= kDescMaxKeypoints, SG_EINVAL, "keypoint count must be 0..2^20");
  SG_REQUIRE(slot >= 0 && slot < (int)slots_.size() && slots_[slot].valid, SG_EINVAL, "empty slot");
  SG_REQUIRE(n == 0 || (xy && desc), SG_EINVAL, "null keypoints or descriptors");
  if (levels)
    for (int i = 0; i < n; ++i)
      SG_REQUIRE(levels[i] >= 0 && levels[i] < opt_.depth, SG_EINVAL, "keypoint level outside the pyramid");
  if (n == 0) return;
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  const Slot& s = slots_[slot];
  DescPyr pyr{};
  for (int l = 0; l < opt_.depth; ++l) {
    pyr.img[l] = s.pyr.ptr + s.off[l];
    pyr.w[l] = s.w[l];
    pyr.h[l] = s.h[l];
  }
  desc_xy_.Resize(2 * (size_t)n);
  desc_lv_.Resize(n);
  desc_out_.Resize(4 * (size_t)n);
  desc_bin_.Resize(n);
  desc_st_.Resize(n);
  SG_HIP_CHECK(hipMemcpyAsync(desc_xy_.ptr, xy, sizeof(float) * 2 * n, hipMemcpyHostToDevice, stream_));
  if (levels)
    SG_HIP_CHECK(hipMemcpyAsync(desc_lv_.ptr, levels, sizeof(int32_t) * n, hipMemcpyHostToDevice, stream_));
  else
    desc_lv_.Zero(stream_);
  SG_HIP_CHECK(hipEventRecord(ev_[4], stream_));
  hipLaunchKernelGGL(k_describe, dim3((n + kDescWaves - 1) / kDescWaves), dim3(64 * kDescWaves), 0, stream_, pyr, n,
                     desc_xy_.ptr, desc_lv_.ptr, desc_out_.ptr, desc_bin_.ptr, desc_st_.ptr);
  SG_HIP_CHECK(hipEventRecord(ev_[5], stream_));
  SG_HIP_CHECK(hipGetLastError());
  SG_HIP_CHECK(hipMemcpyAsync(desc, desc_out_.ptr, sizeof(uint64_t) * 4 * n, hipMemcpyDeviceToHost, stream_));
  if (angle_bin)
    SG_HIP_CHECK(hipMemcpyAsync(angle_bin, desc_bin_.ptr, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream_));
  if (status)
    SG_HIP_CHECK(hipMemcpyAsync(status, desc_st_.ptr, sizeof(int32_t) * n, hipMemcpyDeviceToHost, stream_));
  SG_HIP_CHECK(hipStreamSynchronize(stream_));
  float ms = 0.f;
  SG_HIP_CHECK(hipEventElapsedTime(&ms, ev_[4], ev_[5]));
  describe_ms_ = ms;
}

}  // namespace sg
