// ba_chain.h — the host-only planner of one LM iteration's launch chain: which kernels BaSolver::EnqueueIterations
// (ba_solver.hip) launches, with which mode arguments and in what order, and where the landmark shards all-reduce.
// A pure function of its arguments (no HIP, no environment, no state), so a CPU test can enumerate every regime
// (tests/native/chain_plan_check.cpp).  The driver walks the returned ops and calls ba_launch.h's launchers; the
// grids, buffers, the Cholesky kernel choice and its flag bits stay there.
#ifndef SG_BA_CHAIN_H_
#define SG_BA_CHAIN_H_

#include <cstdint>

namespace sg {

// The switches read once per solver (ReadRunKnobs, ba_solver.hip, from the BaSolver constructor), as plain values.
struct RunKnobs {
  bool spec = true;             // SG_SPEC=0: k_point_update + k_linearize every iteration instead of k_update_lin
  int merge = 1;                // SG_XCHG_MERGE: 1 merged exchange on landmark shards, 0 off, 2 (=force) on one rank too
  bool pack_force = false;      // SG_PACK_S set: pack / unpack S on one rank too (tests the path)
  bool comm_force = false;      // SG_COMM_FORCE=1: issue the communicator's collectives on one rank too (tests)
  bool chol_zpre = true;        // SG_CHOL_ZPRE=0: k_chol_tiles factors D_0 itself, not from k_S_reduce's Z_0 (A/B, tests)
  bool chol_stile = true;       // SG_CHOL_STILE=0: k_chol_tiles loads row-major S, not k_S_reduce's tile-major copy
  bool chol_force_tmo = false;  // SG_CHOL_FORCE_TIMEOUT: the dissected Cholesky's separator wait times out (tests only)
  int chol_delay = 0;           // SG_CHOL_DELAY=bottom|top: 64 | 128, that workgroup of the dissected Cholesky sleeps a
                                // few tens of µs (the bottom before its first phase, the top before its poll), so both
                                // arrival orders of the hand-off run (tests only)
};

// What the chain depends on besides the knobs; fixed from a load to the next.
struct ChainShape {
  bool multi = false;     // landmark shards: more than one rank
  bool assemble = true;   // this rank adds the FrameDistance terms and the damping (no communicator, or rank 0)
  int nk = 0;             // free intrinsics columns (0: none)
  bool tiles = false;     // CholPlan::tiles
  bool border = false;    // CholPlan::border
};

// (The driver's timer table and the check's name table are in this order.)
enum class ChainOp : uint8_t {
  Linearize,       // k_linearize
  CamReduce,       // k_cam_reduce: a = workgroups beyond the camera blocks (1 or 2), b = mode
  Decide,          // k_decide: a = take (1: the pending speculative decision; 0: the two-pass chain's on shards)
  AllReduceCam,    // the camera blocks and cost scalars summed over the shards
  IntrLinearize,   // k_intr_*: the linearization side of the free intrinsics
  CamFinalize,     // k_cam_finalize: a = mode
  Schur,           // k_schur: a = fin (0 none, 1 the finalize pass, 2 its mode 1)
  SReduce,         // k_S_reduce: a = amode, b = pre (bit 0 Z_0 for k_chol_tiles, bit 1 the tile-major copy St)
  IntrSchur,       // k_intr_*: the Schur side
  Exchange,        // pack, all-reduce, unpack of S's band: a = with the merged tail, b = unpack with k_S_unpack_fin
  Chol,            // the Cholesky the load chose: a = zpre, b = stile (k_chol_tiles' flag bits 4 and 5)
  IntrStep,        // k_intr_step
  UpdateLin,       // k_update_lin
  PointUpdate,     // k_point_update
  UpdReduce,       // k_upd_reduce: a = fuse (the decision in the same launch)
  AllReduceUpd,    // the update scalars summed over the shards
  kCount
};

struct ChainCall {
  ChainOp op;
  int8_t a, b;
};

// No step has more ops than this: the check enumerates every input PlanIteration distinguishes.
constexpr int kChainMaxOps = 20;

struct ChainStep {
  ChainCall ops[kChainMaxOps];
  int n = 0;
  bool pending_out = false;   // the step ended with k_cam_reduce mode 1: its decision is the next step's first launch
  bool stile = false;         // k_chol_tiles took the tile-major copy (sg_ba_info.cholesky_stile)
};

// One LM iteration.  first_it: the first of a solve (it fixes the camera scale); pending_in: the previous step's
// pending_out.
ChainStep PlanIteration(const ChainShape& s, const RunKnobs& k, bool first_it, bool pending_in);
// The end of a batch of iterations: no decision stays pending, so the host's state reads and downloads see the
// decided step.
ChainStep PlanBatchTail(bool pending);

}  // namespace sg

#endif  // SG_BA_CHAIN_H_
