// ba_layout.h — what the host planner (ba_plan.cpp) and the bundle-adjustment kernels share: the work-unit
// records, the packed observation word, the sizes the work lists are cut to and the index arithmetic of the
// Schur slabs and the Cholesky's LDS.  No HIP header: it compiles with a plain host compiler too.
#ifndef SG_BA_LAYOUT_H_
#define SG_BA_LAYOUT_H_

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SG_LAYOUT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SG_LAYOUT_HD inline
#endif

namespace sg {

constexpr int kCamV = 27;           // per camera block: upper(Jc^T Jc) 21 + Jc^T r 6
constexpr int kCholNb = 16;

// Packed per-observation facts (device order), so that a sweep lane's loads depend only on its own
// observation record: camera block + 1 (0: frame not free) in bits 0-15, camera in bits 16-23, then the
// frame's rotation / translation freedom, the point's freedom and the fixed flag (all blocks constant).
constexpr int kMetaCamShift = 16;
constexpr int kMetaRot = 1 << 24, kMetaTrans = 1 << 25, kMetaPfree = 1 << 26, kMetaFixed = 1 << 27;
SG_LAYOUT_HD int meta_block(int m) { return (m & 0xffff) - 1; }
SG_LAYOUT_HD int meta_cam(int m) { return (m >> kMetaCamShift) & 0xff; }

// k_schur work decomposition (see ba_plan.cpp): a segment is a run of consecutive points (device order)
// whose camera columns fit a window of <= kSchurTW 16-column tiles of S, one workgroup (kSchurCWaves waves holding
// the window's upper tiles and rhs rows in MFMA accumulators, a point wave, kSchurCellWaves building the
// operand tiles); it streams through
// LDS in batches of <= kSchurBatchPts points whose operand tiles (64 doubles each) fit kSchurXCap.  The cells
// of a point (one per block of its span) carry its observations.  A point spanning more than kSegNbMax blocks
// is a WideSeg of its own (observation pairs, global atomics).
#ifndef SG_SEG_NB
#define SG_SEG_NB 24   // widest point of a segment, in blocks (6 * 24 + 14 <= 16 * kSchurTW columns)
#endif
constexpr int kSegNbMax = SG_SEG_NB;
static_assert(kSegNbMax <= 24, "cells of a batch: kSchurBatchCells");
constexpr int kSchurCellWaves = 3;   // operand-tile waves (a batch has <= 64 kSchurCellWaves cells)
#ifndef SG_SCHUR_CW
#define SG_SCHUR_CW 4
#endif
constexpr int kSchurCWaves = SG_SCHUR_CW;   // MFMA waves (4: one per SIMD; 8: two); a point wave between the groups
constexpr int kSchurWaves = kSchurCellWaves + 1 + kSchurCWaves;
constexpr int kSchurThreads = 64 * kSchurWaves;
#ifndef SG_SCHUR_TW
#define SG_SCHUR_TW 10   // window width in tiles (variant builds: tools/build_variant.sh)
#endif
constexpr int kSchurTW = SG_SCHUR_TW;
constexpr int kSchurTiles = kSchurTW * (kSchurTW + 1) / 2;
constexpr int kSchurAug = kSchurTiles + kSchurTW;   // window tiles + one rhs tile per tile row
constexpr int kSchurTPW = (kSchurAug + kSchurCWaves - 1) / kSchurCWaves;   // accumulator tiles per wave
constexpr int kSchurXCap = 112 * 64;   // operand tiles (64 doubles each) per batch buffer
#ifndef SG_SCHUR_BATCH
#define SG_SCHUR_BATCH 32
#endif
constexpr int kSchurBatchPts = SG_SCHUR_BATCH;   // <= 64: a batch's point table is one point per lane
constexpr int kSchurBatchCells = kSchurBatchPts * 24;   // cells of a batch (spans <= kSegNbMax)
static_assert(6 * kSegNbMax + 14 <= 16 * kSchurTW, "a widest point must fit the tile window");
struct SchurSeg {
  int32_t p0, p1;       // point range
  int32_t b_lo, nb;     // blocks the points observe: rhs partial [b_lo, b_lo + nb)
  int32_t s_off;        // S_slab offset: ntw (ntw + 1) / 2 row-major 16x16 tiles, then 6 nb rhs entries
  int32_t t0, ntw;      // window: tile columns [t0, t0 + ntw) of S
  int32_t bt0, bt1;     // batches
  int32_t pad;
};
struct SchurBatch {
  int32_t p0, p1;       // points
  int32_t c0, c1;       // cells
};
struct WideSeg {
  int32_t p;            // the point
  int32_t pair_lo, pair_hi;
  int32_t pad;
};

// Augmented slot order of a segment window: level c = 0 .. kSchurTW-1 holds the window tiles (0, c) .. (c, c),
// then the rhs tile of tile row c (E_c^T w in its column 0).  A point whose columns end in window tile jhi
// touches exactly the levels <= jhi: a prefix of schur_aug_base(jhi + 1) slots.  Wave W owns slots u = W + 4 s.
SG_LAYOUT_HD constexpr int schur_aug_base(int c) { return c * (c + 3) / 2; }
// window tile t of the segment slab's column-major upper order: its column and row (r <= c)
SG_LAYOUT_HD constexpr int schur_tile_c(int t) {
  int c = 0;
  while ((c + 1) * (c + 2) / 2 <= t) ++c;
  return c;
}
SG_LAYOUT_HD constexpr int schur_tile_r(int t) { return t - schur_tile_c(t) * (schur_tile_c(t) + 1) / 2; }

// k_linearize work decomposition: a chunk (one single-wave workgroup) is a run of consecutive points whose
// camera blocks fit one window of <= kLinNbMax blocks, split into rounds of <= kLinObs observations and
// <= kLinPts points that hold whole points (one observation per lane).  A point with more observations, or
// spanning more blocks, is a "wide" chunk of its own: rounds are pieces of it and its camera terms go to
// global atomics.  A chunk's workgroup has one or two waves (WorkCounts::lin_waves, fixed at load: two when the
// grid would leave SIMDs idle): wave w takes rounds r0 + w, r0 + w + 2, ... into LDS accumulators of its own,
// summed in wave order at the end (a wide chunk runs on wave 0).
constexpr int kLinThreads = 64;   // lanes of one wave (one observation per lane)
constexpr int kLinObs = 64;
constexpr int kLinPts = 16;
constexpr int kLinNbMax = 24;
constexpr int kLinMaxRounds = 4;   // measured best at 130k and 1.6M observations
struct LinRound {
  int32_t o0, o1;     // observation range
  int32_t p0, p1;     // points (whole points; every piece of a wide point names it)
};
struct LinChunk {
  int32_t r0, r1;     // round range
  int32_t b_lo, nb;   // camera window [b_lo, b_lo + nb) (nb = 0: no camera terms in LDS)
  int32_t cam_off;    // offset of this chunk's camera partials in cam_slab (doubles)
  int32_t wide;       // one point: camera terms by global atomics, point block reduced over the workgroup
  int32_t p0, p1;
  int32_t u0;         // its first k_point_update work unit (one per round; one for a wide chunk)
};

// Launch outputs that only a later launch reads, stored write-through (wt_store.h): Dev::wt bits, SG_WT_STORES.
constexpr int kWtJ = 1;       // the J records (jstore / jstore_zero: k_linearize, k_update_lin)
constexpr int kWtCam = 2;     // the per-chunk camera partials (lin_combine_waves)
constexpr int kWtSchur = 4;   // k_schur's segment slabs (schur_store)
constexpr int kWtStoresDefault = kWtJ | kWtCam | kWtSchur;

// ---- the reduced-camera solves (ba_chol.hip): the sizes the Cholesky choice is made by
constexpr int kCholWS = 128;           // k_cholesky_window: LDS window columns
constexpr int kJendSh = 512;           // panel band ends cached in LDS (n <= 8192)
constexpr int kCandMax = 1024;         // frames / FrameDistance residuals staged in LDS for the candidate pass
constexpr int kTB = 8;                 // k_chol_tiles: band width in tiles = waves
constexpr int kTileMaxNT = 400;        // k_chol_tiles: tile rows (dynamic LDS: x, z' 16 NT doubles each + band ends)
constexpr int kSplitMinNT = 13;        // dissected band from this many tile rows
// the candidate pass's operands staged in a Cholesky's LDS (CandLds, ba_chol.hip), bytes
SG_LAYOUT_HD constexpr size_t cand_lds_bytes(int F, int D, int n) {
  return (size_t)(7 * F + n + 7 * D + 3 * F) * sizeof(double) + (size_t)(2 * F + 2 * D) * sizeof(int);
}
// k_chol_border's dynamic LDS (doubles): x [16 NT], z' [16 NT], row flags [NT ints], then (flags bit 0) the q_K
// tiles [256 NT] and (bit 1) the candidate pass's operands (staged by the waves that wait for the chain)
SG_LAYOUT_HD constexpr size_t border_lds_doubles(int NT, int flags, int F, int D, int n) {
  size_t o = 32 * (size_t)NT + (NT + 1) / 2;
  if (flags & 1) o += 256 * (size_t)NT;
  if (flags & 2) o += (cand_lds_bytes(F, D, n) + 7) / 8;
  return o;
}
// St, the tile-major copy of S's band (ba_plan.h: PlanStile): slots of 256 doubles, two per tile of the NT kTB
// band positions (top and bottom workgroup) and one that stays zero; element (a, b) of a slot sits where lane
// 16 (a & 3) + b holds it in register a >> 2 of a k_chol_tiles accumulator.
SG_LAYOUT_HD constexpr size_t stile_doubles(int NT) { return ((size_t)2 * NT * kTB + 1) * 256; }
SG_LAYOUT_HD constexpr int stile_elem(int a, int b) { return 64 * (a >> 2) + 16 * (a & 3) + b; }

}  // namespace sg

#endif  // SG_BA_LAYOUT_H_
