// wt_store.h — write-through (agent-scope, sc1) stores and the matching loads.  A plain store leaves its line
// dirty in the storing XCD's write-back L2 and the launch boundary pays for the write-back; an sc1 store sends the
// bytes out when it issues and drops the line from that L2.  Two uses:
//   * a hand-off inside a launch (k_chol_tiles' separator, ba_chol.hip): st_wt by the producer, ld_wt or an
//     acquire by the consumer;
//   * launch outputs that only a LATER launch reads (Dev::wt, the kWt* bits of ba_layout.h: the sweeps' J records
//     and camera partials, k_schur's segment slabs): the bytes leave while the launch still computes instead of at
//     its end.  The rule for such a buffer: no instruction of the launch that stores it reads those bytes, so the
//     kernel boundary is all the ordering there is — no drain, flag or fence goes with the stores.
// Vector stores only, whole lines per wave instruction: narrow sc1 stores cost several times a 16-byte one per byte.
#ifndef SG_WT_STORE_H_
#define SG_WT_STORE_H_

#include <hip/hip_runtime.h>

namespace sg {

// 8 bytes per lane.
__device__ __forceinline__ void st_wt(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_wt(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 16 bytes per lane at p + kByteOff (an instruction offset, -4096 .. 4095, so several stores share one address).
// p is a global address, 16-byte aligned.  The nop keeps the next instruction off the data registers while the
// store still reads them (the compiler does not know this instruction's hazards).
typedef double wt_f64x2 __attribute__((ext_vector_type(2)));
template <int kByteOff>
__device__ __forceinline__ void st_wt16(const void* p, double x, double y) {
  static_assert(kByteOff >= -4096 && kByteOff <= 4095 && kByteOff % 16 == 0, "instruction offset range");
  wt_f64x2 v;
  v.x = x;
  v.y = y;
  asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1\n\ts_nop 1" : : "v"(p), "v"(v), "n"(kByteOff) : "memory");
}

}  // namespace sg

#endif  // SG_WT_STORE_H_
