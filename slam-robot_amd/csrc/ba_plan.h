// ba_plan.h — the host-only planner of a full sg_ba_load: everything the kernels read that is a function of the
// problem's structure alone.  Pure functions of their arguments (no HIP, no environment, no state, no I/O), so a
// CPU test can check what the kernels' comments promise (tests/native/ba_plan_check.cpp).  BaSolver::Load
// (ba_solver.hip) calls the stages in the order below, uploads their outputs and sizes the device buffers.
//
//   order      PlanBlocks, PlanPointOrder, PlanObservations         -> Order
//   work lists PlanSweep, PlanSchur, PlanReduceLists, PlanFrameDistance, PlanIntrLists, PlanLoBlk -> WorkLists
//   envelope   PlanEnvelope (from the envelope of every rank's points: Load all-reduces lo_blk before it)
//   Cholesky   PlanChol: which of the four kernels factors S, and the dissected band's split
//
// A list a kernel reads even when it has no entries is padded here to one element; the counts beside the lists
// say how many entries are real.
#ifndef SG_BA_PLAN_H_
#define SG_BA_PLAN_H_

#include <cstddef>
#include <cstdint>
#include <vector>

#include "ba_layout.h"
#include "slamgpu.h"

namespace sg {

// The knobs read at every full load (ReadLoadKnobs, ba_solver.hip), as plain values.
struct LoadKnobs {
  int lin_waves = 0;          // SG_LIN_WAVES: 0 unset (chosen by the chunk count), else 1 or 2
  bool chol_gstage = true;    // SG_CHOL_GSTAGE=0: k_cholesky_global never stages its panel rows in LDS
  bool chol_window = false;   // SG_CHOL_WINDOW set: no tiled kernel
  bool chol_border = true;    // SG_CHOL_BORDER=0: free intrinsics on the arrowhead k_cholesky_global
  bool chol_split = true;     // SG_CHOL_SPLIT=0: no dissected band
  bool chol_sep7 = false;     // SG_CHOL_SEP=7: the fixed 7-row separator
  bool stamp = false;         // SG_STAMP=1: cycle stamps
  int wt_stores = kWtStoresDefault;   // SG_WT_STORES: kWt* bits (ba_layout.h), launch outputs stored write-through
};

// Camera blocks and the device order of points and observations.
struct Order {
  int F = 0, P = 0, M = 0, D = 0;
  int NB = 0;   // camera blocks: the frames with a free rotation or translation
  int nk = 0;   // 7 * cameras when the intrinsics are free
  int n = 0;    // columns of S: 6 NB frame columns, then the free intrinsics
  std::vector<int32_t> frame_block;   // [F] block of a frame, -1: constant
  std::vector<int32_t> point_perm;    // device order -> problem point: by first free block, none last (stable)
  std::vector<int32_t> inv_perm;
  std::vector<int32_t> dfirst, dlast; // [P] first / last free block of a point in device order (NB / -1: none)
  std::vector<int32_t> poff;          // [P + 1] observations, CSR by device point
  std::vector<int32_t> obs_perm;      // device order -> problem observation: within a point by block, constant
                                      // frames first (stable)
  // device-order copies of the problem's arrays
  std::vector<double> X, obs_pt;
  std::vector<uint8_t> pfree, obs_fixed;
  std::vector<int32_t> obs_frame;
  std::vector<int32_t> obs_meta;      // [max(M, 1)] kMeta* words
};
void PlanBlocks(const sg_problem& p, Order* o);
void PlanPointOrder(const sg_problem& p, Order* o);
void PlanObservations(const sg_problem& p, Order* o);

// The scalars of the work lists (what BaSolver keeps of them after the upload).
struct WorkCounts {
  int nlin = 0;          // sweep chunks
  int lin_waves = 1;     // waves per k_linearize / k_update_lin chunk (2 when 2 nlin waves fit the chip at once)
  int npu = 0;           // k_point_update work units
  int lcam_off = 0;      // doubles of one cam_slab slot
  int ncell = 0, nseg = 0, nwide = 0;
  int s_off = 0;         // doubles of S_slab
  int r_lstride = 256;   // k_S_reduce's padded r_lidx rows (Dev::r_lstride)
  int intr_nsl = 1;      // k_intr_fk workgroups per block list
  size_t npairs = 0;     // Schur observation pairs
  double schur_mfma = 0.0;    // v_mfma_f64_16x16x4f64 tile updates per k_schur launch (KernelWork)
  double schur_rhs = 0.0;     // v_mfma_f64_4x4x4_4b_f64 rhs updates per k_schur launch
  double schur_useful = 0.0;  // flops of the slots that multiply each point's own tiles (no zero tiles)
};
struct WorkLists : WorkCounts {
  std::vector<LinChunk> lchunks;
  std::vector<LinRound> lrounds;
  std::vector<int32_t> pu_units;   // a round index, or -(chunk + 1) for wide chunks
  std::vector<int32_t> pinfo, pmx, cells, cell_obs;   // Dev::pinfo, pmx, cells, cell_obs
  std::vector<SchurSeg> segs;      // [max(nseg, 1)]
  std::vector<SchurBatch> sbatch;
  std::vector<WideSeg> wsegs;      // [max(nwide, 1)]
  std::vector<int32_t> pairs;      // int2 per pair (wide points)
  std::vector<int32_t> cam_loff, cam_lidx, r_loff, r_lidx;   // the deterministic reduce lists
  std::vector<int32_t> fd_a, fd_b, fd_boff, fd_bidx, fd_pair;
  std::vector<int32_t> intr_boff, intr_bidx;   // free intrinsics only
  std::vector<int32_t> lo_blk;     // [NB] first block row of block column J's envelope, this rank's points
};
void PlanSweep(const Order& o, int ncu, int lin_waves_knob, WorkLists* w);
void PlanSchur(const Order& o, int ncu, WorkLists* w);
void PlanReduceLists(const Order& o, WorkLists* w);
void PlanFrameDistance(const sg_problem& p, const Order& o, WorkLists* w);
void PlanIntrLists(const Order& o, WorkLists* w);
void PlanLoBlk(const Order& o, WorkLists* w);

struct EnvCounts {
  int npanel = 0;
  int band_tiles = 0;    // widest Cholesky envelope row (16-wide tiles)
  int nstile = 0;        // band tiles of the frame columns (k_S_reduce)
  int s_lstride = 256;   // its padded s_lidx rows (Dev::s_lstride)
  size_t npack = 0;      // band of S + rhs, doubles (all-reduce size)
};
struct Envelope : EnvCounts {
  // [npanel] band end of each 16-row panel (16-aligned or n); with free intrinsics every panel reaches n and
  // the frame band ends (panel_bend) follow as a tail
  std::vector<int32_t> panel_jmax;
  std::vector<int32_t> pack_off;   // [npanel + 1] offset of a panel's band rows in the packed all-reduce buffer
  std::vector<int32_t> stile, s_loff, s_lidx;   // Dev::stile, s_loff, s_lidx
};
Envelope PlanEnvelope(const Order& o, const std::vector<int32_t>& lo_blk, const std::vector<SchurSeg>& segs,
                      int nseg);

// The dynamic LDS granted to k_chol_tiles, k_cholesky_global and k_chol_border (CholSetAttributes).
struct CholGrants {
  size_t tiles = 0, global = 0, border = 0;
};
struct CholPlan {
  bool window = true;     // k_cholesky_window (band ends cached in LDS), else k_cholesky_global
  bool tiles = false;     // tiled register-resident band Cholesky (k_chol_tiles)
  bool border = false;    // free intrinsics: k_chol_tiles on the frame band, then k_chol_border
  int border_flags = 0;   // its LDS placements (bit 0 q_K tiles, bit 1 candidate operands)
  bool gstage = false;    // k_cholesky_global stages panel rows in LDS
  bool cand_lds = false;  // candidate-pass operands staged in k_chol_tiles' LDS (small problems)
  size_t tile_lds = 0;    // k_chol_tiles' dynamic LDS
  int nd = 0;             // dissected band: tile rows the second workgroup factors bottom-up (0: one WG)
  int ns = kTB - 1;       // ... and the separator's tile rows (<= 7)
  size_t wg_size = 0;     // doubles of k_chol_tiles' W buffer (0: not tiled)
};
CholPlan PlanChol(const Order& o, const Envelope& e, const CholGrants& g, const LoadKnobs& k);

// St, the tile-major copy of S's band that k_S_reduce writes beside S and k_chol_tiles loads its tiles from: slots of
// 256 doubles in the accumulator layout (lane l = 16 lk + li, register q at 256 slot + 64 q + l: element (lk + 4q,
// li)), each workgroup's tiles in its own factor order.
//   top half, slots [0, NT kTB): slot I kTB + (J - I) is tile (I, J) of S, for the rows and columns the top
//     workgroup factors (all of S without a split, < m + ns with one);
//   bottom half, slots [NT kTB, 2 NT kTB): slot NT kTB + I' kTB + (J' - I') is tile (I', J') of P S P (index i ->
//     16 NT - 1 - i), rows I' < nd: S tile (R, C) = (NT-1-J', NT-1-I'), C >= m + ns, element (a, b) -> (15-b, 15-a);
//   slot 2 NT kTB: never written (zero), what a load of a tile outside a workgroup's rows or columns reads.
// Band tiles get one slot each (the separator block belongs to the top only: the bottom starts it at zero); the
// other slots stay zero from the load.  Padding past n is written as the identity.  (stile_doubles, stile_elem:
// ba_layout.h)
struct StilePlan {
  std::vector<int32_t> dst;        // [max(nstile, 1)][2] per Envelope::stile entry: top slot or -1, bottom slot or -1
  std::vector<int32_t> tend_rev;   // [NT] band end (tiles, exclusive, unclamped) of row k of P S P: NT - lo(NT-1-k),
                                   // lo(c) the first tile row of S whose band covers column c
};
StilePlan PlanStile(const Envelope& e, const CholPlan& c);

}  // namespace sg

#endif  // SG_BA_PLAN_H_
