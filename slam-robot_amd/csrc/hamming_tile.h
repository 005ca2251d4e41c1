// hamming_tile.h — the device pieces that hamming.hip (all pairs) and retrieve.hip (a query against every keyframe of
// a database) share: the +-1 int8 expansion of descriptor bits, the matrix-core tile that leaves 2 h in every element
// of a 16 x 16 (query x train) block, and the slice body that runs 256 queries against one run of train descriptors.
// The key rule is best2.h's.  See hamming.hip for the formulation.  Device code only; included inside a HIP
// translation unit.
#ifndef SG_HAMMING_TILE_H_
#define SG_HAMMING_TILE_H_

#include <hip/hip_runtime.h>

#include "best2.h"

namespace sg {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));   // 16 int8 (one MFMA A/B fragment) or 4 int32 (C/D)

constexpr int kHmThreads = 512;              // 8 waves: 4 query groups x 2 train halves
constexpr int kHmQ = 256;                    // queries per workgroup
constexpr int kHmTile = 128;                 // train descriptors per LDS tile
constexpr int kHmPitch = 272;                // LDS bytes per descriptor row (256 + 16)
constexpr int kKeyShift = kBest2Shift;       // slice index bits of the packed key (slices <= 2^22)

// 4 bits -> 4 bytes of +-1: spread bit i to byte i ((n * 0x204081) & 0x01010101, no carries: the shifted
// copies do not overlap), make each set byte 0xFF ((s << 8) - s), then pick +1 / -1 per byte with v_bfi.
// pos: the byte of a set bit (+1 for queries, -1 for the train side); the clear bits get the other sign.
__device__ __forceinline__ int expand4(unsigned nib, unsigned pos, unsigned negv) {
  const unsigned s = __umul24(nib, 0x204081u) & 0x01010101u;
  const unsigned m = (s << 8) - s;
  return (int)((m & pos) | (~m & negv));   // v_bfi_b32
}
// 16 bits -> one A/B fragment (16 int8)
__device__ __forceinline__ v4i expand16(unsigned b, unsigned pos, unsigned negv) {
  v4i w;
  w[0] = expand4(b & 15u, pos, negv);
  w[1] = expand4((b >> 4) & 15u, pos, negv);
  w[2] = expand4((b >> 8) & 15u, pos, negv);
  w[3] = expand4((b >> 12) & 15u, pos, negv);
  return w;
}

// qb / tb: the descriptors' bits, 16 uint16 (256 bits) per descriptor; expanded to +-1 int8 on the way in
// (A fragments once per workgroup, B tiles into LDS).
template <bool kPartial>
__device__ __forceinline__ void ham_tile(const v4i (&a)[4][4], const unsigned char* tile, int wi, int li, int g,
                                         int tbase, int cnt, unsigned (&m1)[4][4], unsigned (&m2)[4][4]) {
  const v4i cinit = {256, 256, 256, 256};
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int row = 64 * wi + 16 * ct + li;
    v4i acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const v4i bf = *reinterpret_cast<const v4i*>(tile + row * kHmPitch + 64 * k + 16 * g);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
        acc[rt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[rt][k], bf, k == 0 ? cinit : acc[rt], 0, 0, 0);
    }
    // acc[rt][r] = 2 h of query 16 rt + 4 g + r and train descriptor tbase + row (slice index)
    const unsigned idx = (unsigned)(tbase + row);
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        unsigned key = ((unsigned)acc[rt][r] << kKeyShift) | idx;
        if (kPartial) key = (int)idx < cnt ? key : kBest2Inf;
        Best2Take(key, m1[rt][r], m2[rt][r]);
      }
  }
}

// One workgroup's slice: queries 256 qgroup .. + 255 of qb[nq] against train descriptors j0 .. j0 + cnt - 1 of tb,
// streamed through the LDS tile.  Every thread of the workgroup calls it (it holds barriers).  Where `write` comes
// back set, q < nq is this lane's query and (k1, k2) its best and second key of the slice, with slice-local indices in
// the keys (kBest2Inf where the slice has no such descriptor); the lanes of the second train half and those past nq
// do not write.
struct HamSliceKeys {
  int q;
  unsigned k1, k2;
  bool write;
};
__device__ __forceinline__ HamSliceKeys ham_slice(const uint16_t* __restrict__ qb, int nq,
                                                  const uint16_t* __restrict__ tb, int j0, int cnt, int qgroup,
                                                  unsigned char* tile, unsigned (&red)[4][64][2]) {
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wq = wave & 3, wi = wave >> 2;
  const int qbase = qgroup * kHmQ + 64 * wq;
  // A fragments: row tile rt, K-step k: query qbase + 16 rt + li, bytes 64 k + 16 g
  v4i a[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt) {
    const int qi = min(qbase + 16 * rt + li, nq - 1);   // nq >= 1 (nothing is launched for nq == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) a[rt][k] = expand16(qb[(size_t)qi * 16 + 4 * k + g], 0x01010101u, 0xFFFFFFFFu);
  }
  unsigned m1[4][4], m2[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) m1[rt][r] = m2[rt][r] = kBest2Inf;
  const int ntile = (cnt + kHmTile - 1) / kHmTile;
  // tile loads: 128 descriptors x 16 chunks of 16 bits, 4 chunks per thread (chunk c: descriptor c >> 4,
  // bits 16 (c & 15) ..); descriptors past the slice end read the slice's last one (masked in the epilogue), so no
  // load leaves the slice; each chunk is expanded to a 16-byte fragment (train side: set bit -> -1) on its way into
  // LDS
  unsigned pre[4];
  auto load_tile = [&](int t) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = tid + kHmThreads * u;
      const int item = min(t * kHmTile + (c >> 4), cnt - 1);
      pre[u] = tb[(size_t)(j0 + item) * 16 + (c & 15)];
    }
  };
  if (ntile > 0) load_tile(0);   // (cnt == 0, an empty train set: no descriptor to read)
  for (int t = 0; t < ntile; ++t) {
    __syncthreads();   // the previous tile's fragments are read
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = tid + kHmThreads * u;
      *reinterpret_cast<v4i*>(tile + (c >> 4) * kHmPitch + 16 * (c & 15)) = expand16(pre[u], 0xFFFFFFFFu, 0x01010101u);
    }
    __syncthreads();
    if (t + 1 < ntile) load_tile(t + 1);
    if ((t + 1) * kHmTile > cnt)
      ham_tile<true>(a, tile, wi, li, g, t * kHmTile, cnt, m1, m2);
    else
      ham_tile<false>(a, tile, wi, li, g, t * kHmTile, cnt, m1, m2);
  }
  // merge over the 16 tile columns (lanes of a 16-lane group)
#pragma unroll
  for (int mask = 1; mask < 16; mask <<= 1)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned o1 = __shfl_xor(m1[rt][r], mask), o2 = __shfl_xor(m2[rt][r], mask);
        Best2Merge(m1[rt][r], m2[rt][r], o1, o2);
      }
  // lane li of group g takes query 16 (li >> 2) + 4 g + (li & 3) of the wave's 64
  unsigned k1 = kBest2Inf, k2 = kBest2Inf;
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (li == 4 * rt + r) {
        k1 = m1[rt][r];
        k2 = m2[rt][r];
      }
  const int ql = 16 * (li >> 2) + 4 * g + (li & 3);
  if (wi == 1) {
    red[wq][ql][0] = k1;
    red[wq][ql][1] = k2;
  }
  __syncthreads();
  const int q = qbase + ql;
  if (wi == 1) return HamSliceKeys{q, k1, k2, false};
  Best2Merge(k1, k2, red[wq][ql][0], red[wq][ql][1]);
  return HamSliceKeys{q, k1, k2, q < nq};
}

}  // namespace

}  // namespace sg

#endif  // SG_HAMMING_TILE_H_
