// hamming_tile.h — the device pieces that hamming.hip (all pairs) and retrieve.hip (a query against every keyframe of
// a database) share: the +-1 int8 expansion of descriptor bits, the packed-key arg-min rule, and the matrix-core tile
// that leaves 2 h in every element of a 16 x 16 (query x train) block.  See hamming.hip for the formulation.  Device
// code only; included inside a HIP translation unit.
#ifndef SG_HAMMING_TILE_H_
#define SG_HAMMING_TILE_H_

#include <hip/hip_runtime.h>

namespace sg {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));   // 16 int8 (one MFMA A/B fragment) or 4 int32 (C/D)

constexpr int kHmThreads = 512;              // 8 waves: 4 query groups x 2 train halves
constexpr int kHmQ = 256;                    // queries per workgroup
constexpr int kHmTile = 128;                 // train descriptors per LDS tile
constexpr int kHmPitch = 272;                // LDS bytes per descriptor row (256 + 16)
constexpr int kKeyShift = 22;                // slice index bits of the packed key (slices <= 2^22)
constexpr unsigned kKeyInf = 0xFFFFFFFFu;

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

__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) {
  unsigned r;
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

__device__ __forceinline__ void ham_take(unsigned key, unsigned& m1, unsigned& m2) {
  m2 = umed3(m1, key, m2);   // second smallest (m1 <= m2)
  m1 = min(m1, key);
}

__device__ __forceinline__ void ham_merge(unsigned& m1, unsigned& m2, unsigned o1, unsigned o2) {
  const unsigned n2 = min(max(m1, o1), min(m2, o2));
  m1 = min(m1, o1);
  m2 = n2;
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
        if (kPartial) key = (int)idx < cnt ? key : kKeyInf;
        ham_take(key, m1[rt][r], m2[rt][r]);
      }
  }
}

}  // namespace

}  // namespace sg

#endif  // SG_HAMMING_TILE_H_
