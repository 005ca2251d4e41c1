// describe_math.h — the arithmetic of sg_tracker_describe (include/slamgpu.h), shared by the device kernel
// (describe.hip) and the CPU check (tests/native/describe_math_check.cpp), so that the two cannot drift apart:
// the keypoint's centre on its level and the border rule, the disc of the intensity centroid, the order of the
// moment sums, the orientation bin, and a plain per-keypoint CPU function.
//
// The descriptor is a steered BRIEF on one already blurred pyramid level: the orientation is the direction of the
// intensity centroid (m10, m01) of the radius-15 disc around the centre pixel, quantised to 32 bins; the 256 bits
// are pixel-pair comparisons at the integer offsets of brief_pattern.h's table for that bin.  Everything but the
// bin decision is exact: the moments are fp64 sums of exact products in a fixed order, the bits are comparisons
// of stored floats.
#ifndef SG_DESCRIBE_MATH_H_
#define SG_DESCRIBE_MATH_H_

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "brief_pattern.h"

#if defined(__HIPCC__)
#define SG_DESC_HD __host__ __device__ __forceinline__
#else
#define SG_DESC_HD inline
#endif

namespace sg {

constexpr int kDescRadius = 15;                       // disc radius and border, level pixels
constexpr int kDescPatch = 2 * kDescRadius + 1;       // 31: the patch a keypoint reads, row pitch of its copy
constexpr int kDescDiscCount = 709;                   // pixels (u, v) with u^2 + v^2 <= 15^2
constexpr int kDescLanes = 64;
constexpr int kDescPerLane = (kDescDiscCount + kDescLanes - 1) / kDescLanes;   // 12 (lanes 0..4), the rest 11
constexpr int kDescMaxKeypoints = 1 << 20;
constexpr int kDescOk = 0, kDescBorder = 1;           // sg_describe_status

// The disc's offsets in row-major order, padded to 64 * 12 with (0, 0): a padding entry adds the exact product
// 0 * I = +0 to a sum, which changes no bit of it.
struct DescDisc {
  int8_t u[kDescLanes * kDescPerLane], v[kDescLanes * kDescPerLane];
};
constexpr DescDisc MakeDescDisc() {
  DescDisc d{};
  int n = 0;
  for (int v = -kDescRadius; v <= kDescRadius; ++v)
    for (int u = -kDescRadius; u <= kDescRadius; ++u)
      if (u * u + v * v <= kDescRadius * kDescRadius) {
        d.u[n] = (int8_t)u;
        d.v[n] = (int8_t)v;
        ++n;
      }
  return d;
}
static constexpr DescDisc kDescDisc = MakeDescDisc();
constexpr int DescDiscSize() {
  int n = 0;
  for (int v = -kDescRadius; v <= kDescRadius; ++v)
    for (int u = -kDescRadius; u <= kDescRadius; ++u) n += (u * u + v * v <= kDescRadius * kDescRadius) ? 1 : 0;
  return n;
}
static_assert(DescDiscSize() == kDescDiscCount, "the radius-15 disc has 709 pixels");

// Centre pixel of level-0 point (x, y) on level l: px = x 2^-l in fp32 (exact), c = floor(px + 0.5).  False
// (SG_DESC_BORDER) when a coordinate is not finite or the 31 x 31 patch around the centre leaves the w x h level.
// The range test is made on the float, so that no out-of-range value is converted to int.
SG_DESC_HD bool DescCentre(float x, float y, int level, int w, int h, int* cx, int* cy) {
  const float s = 1.0f / (float)(1 << level);
  const float fx = floorf(x * s + 0.5f), fy = floorf(y * s + 0.5f);
  const bool ok = fx >= (float)kDescRadius && fx <= (float)(w - 1 - kDescRadius) && fy >= (float)kDescRadius &&
                  fy <= (float)(h - 1 - kDescRadius);   // false for NaN; an infinity fails its side
  *cx = ok ? (int)fx : 0;
  *cy = ok ? (int)fy : 0;
  return ok;
}

// One term of a moment sum: acc + c * I.  c is an integer of at most four bits and I a float, so the product is
// exact in fp64 and the fused and the unfused form round alike.
SG_DESC_HD double DescAcc(double acc, int c, float I) { return __builtin_fma((double)c, (double)I, acc); }

// The orientation bin of the centroid (m10, m01), image y pointing down: 0 for a zero centroid, else the k whose
// direction 2 pi k / 32 is nearest, as the argmax of the projection m10 cos_k + m01 sin_k formed as
// fma(m10, cos_k, m01 * sin_k), ties to the lower k.  No libm call: one multiplication and one fma per bin.
SG_DESC_HD int DescBin(double m10, double m01) {
  if (m10 == 0.0 && m01 == 0.0) return 0;
  int best = 0;
  double bv = __builtin_fma(m10, kBriefCos[0], m01 * kBriefSin[0]);
  for (int k = 1; k < kBriefBins; ++k) {
    const double v = __builtin_fma(m10, kBriefCos[k], m01 * kBriefSin[k]);
    if (v > bv) {
      bv = v;
      best = k;
    }
  }
  return best;
}

// The moment sums' order: lane l of 64 adds the disc pixels l, l + 64, ... in that order (DescAcc from 0), and the
// 64 partials are added as a balanced pairwise tree over neighbouring lanes (lanes 2i and 2i + 1, then pairs of
// pairs, ...): what wave_sum_full of ba_device.h computes in every lane.
inline double DescTreeSum(const double* part) {
  double t[kDescLanes];
  for (int l = 0; l < kDescLanes; ++l) t[l] = part[l];
  for (int n = kDescLanes; n > 1; n /= 2)
    for (int i = 0; i < n / 2; ++i) t[i] = t[2 * i] + t[2 * i + 1];
  return t[0];
}

// The contract on one keypoint, plainly, on a packed w x h level: status, angle_bin (-1 when refused) and the four
// descriptor words (zero when refused).
inline int DescribeOne(const float* img, int w, int h, int level, float x, float y, uint64_t desc[4],
                       int32_t* angle_bin) {
  desc[0] = desc[1] = desc[2] = desc[3] = 0;
  *angle_bin = -1;
  int cx, cy;
  if (!DescCentre(x, y, level, w, h, &cx, &cy)) return kDescBorder;
  double p10[kDescLanes], p01[kDescLanes];
  for (int l = 0; l < kDescLanes; ++l) {
    double a = 0.0, b = 0.0;
    for (int k = 0; k < kDescPerLane; ++k) {
      const int i = l + kDescLanes * k, u = kDescDisc.u[i], v = kDescDisc.v[i];
      const float I = img[(size_t)(cy + v) * w + (cx + u)];
      a = DescAcc(a, u, I);
      b = DescAcc(b, v, I);
    }
    p10[l] = a;
    p01[l] = b;
  }
  const int bin = DescBin(DescTreeSum(p10), DescTreeSum(p01));
  for (int j = 0; j < kBriefTests; ++j) {
    const int8_t* t = kBriefPattern[bin][j];
    const float a = img[(size_t)(cy + t[1]) * w + (cx + t[0])], b = img[(size_t)(cy + t[3]) * w + (cx + t[2])];
    if (a < b) desc[j >> 6] |= 1ull << (j & 63);
  }
  *angle_bin = bin;
  return kDescOk;
}

}  // namespace sg

#endif  // SG_DESCRIBE_MATH_H_
