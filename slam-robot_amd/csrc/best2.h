// best2.h — the packed-key best / second-best rule of every descriptor matcher (hamming.hip, retrieve.hip,
// ba_match.hip, ba_epipolar.hip), stated once.  Host and device: plain C++ under g++, so a CPU test checks it
// exhaustively (tests/native/best2_check.cpp).
//
// A candidate is one 32-bit key, (distance << kBest2Shift) | index: a smaller key is a smaller (distance, index), so
// ties in distance go to the lower index.  A running answer is the pair m1 <= m2 of the smallest and second smallest
// key seen, kBest2Inf where there is none.  The keys of one query are distinct (the indices are), so (m1, m2) is the
// (min, second min) of the set of keys taken, whatever the order in which they were taken (Best2Take) or in which
// partial answers were combined (Best2Merge): results are reproducible although the order of evaluation is not.
#ifndef SG_BEST2_H_
#define SG_BEST2_H_

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SG_B2_HD __host__ __device__ __forceinline__
#else
#define SG_B2_HD inline
#endif

namespace sg {

constexpr int kBest2Shift = 22;   // index bits of the key: indices < 2^22, distances < 2^10
constexpr uint32_t kBest2Inf = 0xFFFFFFFFu;
constexpr uint32_t kBest2IndexMask = (1u << kBest2Shift) - 1;

SG_B2_HD uint32_t Best2Min(uint32_t a, uint32_t b) { return a < b ? a : b; }
SG_B2_HD uint32_t Best2Max(uint32_t a, uint32_t b) { return a < b ? b : a; }

// One more key.  The new m2 is the median of (m1, key, m2); with m1 <= m2 that is min(m2, max(m1, key)), so the
// device's v_med3_u32 and the host's expression are equal.
SG_B2_HD void Best2Take(uint32_t key, uint32_t& m1, uint32_t& m2) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(m2) : "v"(m1), "v"(key), "v"(m2));
#else
  m2 = Best2Min(m2, Best2Max(m1, key));
#endif
  m1 = Best2Min(m1, key);
}

// The answer over the union of two disjoint key sets from their answers.
SG_B2_HD void Best2Merge(uint32_t& m1, uint32_t& m2, uint32_t o1, uint32_t o2) {
  const uint32_t n2 = Best2Min(Best2Max(m1, o1), Best2Min(m2, o2));
  m1 = Best2Min(m1, o1);
  m2 = n2;
}

// Hamming distance of two 256-bit descriptors given as 128-bit halves with members x, y, z, w (uint4 on the device).
template <typename V>
SG_B2_HD uint32_t Hamming256(const V& a0, const V& a1, const V& b0, const V& b1) {
  return __builtin_popcount(a0.x ^ b0.x) + __builtin_popcount(a0.y ^ b0.y) + __builtin_popcount(a0.z ^ b0.z) +
         __builtin_popcount(a0.w ^ b0.w) + __builtin_popcount(a1.x ^ b1.x) + __builtin_popcount(a1.y ^ b1.y) +
         __builtin_popcount(a1.z ^ b1.z) + __builtin_popcount(a1.w ^ b1.w);
}

// A finished (m1, m2, count) as the four values the matchers return per query.
struct Best2Result {
  int32_t index, best, second, count;   // -1 where there is no such candidate
};
SG_B2_HD Best2Result Best2Decode(uint32_t m1, uint32_t m2, uint32_t count) {
  Best2Result r;
  r.index = m1 == kBest2Inf ? -1 : (int32_t)(m1 & kBest2IndexMask);
  r.best = m1 == kBest2Inf ? -1 : (int32_t)(m1 >> kBest2Shift);
  r.second = m2 == kBest2Inf ? -1 : (int32_t)(m2 >> kBest2Shift);
  r.count = (int32_t)count;
  return r;
}

// What the host requires of a query's four downloaded values before it hands them on: count candidates of at most
// max_count, a best one exactly when there is a candidate and a second exactly when there are two, indices below
// max_index, distances of 256-bit descriptors in order.
SG_B2_HD bool Best2ResultOk(int32_t best_index, int32_t best_dist, int32_t second_dist, int32_t count,
                            int32_t max_index, int32_t max_count) {
  if (!(count >= 0 && count <= max_count && (count == 0) == (best_index < 0) && (count < 2) == (second_dist < 0)))
    return false;
  if (!(best_index < 0 ? best_index == -1 && best_dist == -1
                       : best_index < max_index && best_dist >= 0 && best_dist <= 256))
    return false;
  return second_dist < 0 ? second_dist == -1 : second_dist >= best_dist && second_dist <= 256;
}

#if defined(__HIPCC__)

// The device pieces the two window matchers (k_match_window / k_match_merge, k_epi_window / k_epi_merge) share.  A
// partial answer travels as uint4 (m1, m2, count, 0).

// The waves of a workgroup hold answers for the same 64 queries (lane = query): waves 1 .. kWaves - 1 write theirs to
// wpart, and wave 0 merges them in wave order.  True in wave 0, whose (m1, m2, wn) is then the workgroup's.  Every
// thread of the workgroup calls it.
template <int kWaves>
__device__ __forceinline__ bool Best2MeetWaves(uint4 (&wpart)[kWaves - 1][64], int wave, int lane, uint32_t& m1,
                                               uint32_t& m2, uint32_t& wn) {
  if (wave > 0) wpart[wave - 1][lane] = make_uint4(m1, m2, wn, 0u);
  __syncthreads();
  if (wave > 0) return false;
#pragma unroll
  for (int w = 0; w < kWaves - 1; ++w) {
    const uint4 o = wpart[w][lane];
    Best2Merge(m1, m2, o.x, o.y);
    wn += o.z;
  }
  return true;
}

// A query's ns slices part[first + s * stride], merged in slice order, eight loads a trip.
__device__ __forceinline__ void Best2MergeSlices(const uint4* __restrict__ part, size_t first, size_t stride, int ns,
                                                 uint32_t& m1, uint32_t& m2, uint32_t& wn) {
  m1 = m2 = kBest2Inf;
  wn = 0;
  for (int s0 = 0; s0 < ns; s0 += 8) {
    uint4 p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = part[first + (size_t)min(s0 + u, ns - 1) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (s0 + u >= ns) break;
      Best2Merge(m1, m2, p[u].x, p[u].y);
      wn += p[u].z;
    }
  }
}

// Query k's values into the four rows of out[4 n]: index, best distance, second distance, count.
__device__ __forceinline__ void Best2Store(int32_t* __restrict__ out, size_t n, size_t k, const Best2Result& r) {
  out[k] = r.index;
  out[n + k] = r.best;
  out[2 * n + k] = r.second;
  out[3 * n + k] = r.count;
}

#endif  // __HIPCC__

}  // namespace sg

#endif  // SG_BEST2_H_
