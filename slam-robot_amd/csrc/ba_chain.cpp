// ba_chain.cpp — the launch chain of one LM iteration, planned on the host alone (ba_chain.h).
#include "ba_chain.h"

namespace sg {

static void Push(ChainStep* st, ChainOp op, int a = 0, int b = 0) {
  st->ops[st->n++] = ChainCall{op, (int8_t)a, (int8_t)b};
}

ChainStep PlanIteration(const ChainShape& s, const RunKnobs& k, bool first_it, bool pending_in) {
  ChainStep st;
  // Landmark shards exchange twice per LM iteration after a solve's first: k_S_reduce assembles each rank's own
  // camera blocks (and, on rank 0, the FrameDistance terms) into its partial S, and the camera gradient, diagonal
  // and cost scalars ride in the same all-reduce as the band of S (k_cam_finalize modes 1 and 2); the first
  // iteration sums the camera blocks first (the Jacobi scale of the camera columns comes from them), then S.
  // merge 0: the three-exchange chain every iteration; 2: the merged chain on one rank too (tests the path).
  const bool merged = !first_it && s.nk == 0 && (k.merge == 2 || (s.multi && k.merge == 1));
  // Speculative chain, where the finalize pass runs:
  //   one rank (no free intrinsics): the previous iteration's reduce took the decision (k_cam_reduce mode 2) and
  //     the pass runs inside the k_schur launch;
  //   merged shards: its mode 1 inside the k_schur launch and its mode 2 inside the unpack after the band exchange
  //     (k_S_unpack_fin): two single-workgroup launches of the replicated chain less per iteration;
  //   elsewhere (a solve's first iteration, unmerged shards, free intrinsics, the two-pass chain): k_cam_finalize.
  const bool fin_in_schur = k.spec && !first_it && !s.multi && s.nk == 0 && !merged;
  const bool fin1_in_schur = k.spec && merged;
  // ... and who decides: the closing k_cam_reduce itself on one rank (mode 2; no free intrinsics, no forced merged
  // chain); elsewhere it leaves the candidate's camera reduce and the update scalars (mode 1, + their all-reduce on
  // shards) and the decision pending.
  const bool decide_in_reduce = !s.multi && s.nk == 0 && k.merge != 2;

  // A pending decision is settled first, as its own small launch (k_decide, which also makes an accepted
  // candidate's blocks current).  The driver never leaves one pending before a solve's first iteration, on the
  // two-pass chain, or where the reduce decides.
  if (pending_in) Push(&st, ChainOp::Decide, 1);
  // Speculative mode: only a solve's first iteration linearizes and reduces the camera blocks here; later ones find
  // the linearization of the accepted point in the slot k_update_lin filled, reduced by the closing k_cam_reduce.
  if (!k.spec || first_it) {
    Push(&st, ChainOp::Linearize);
    Push(&st, ChainOp::CamReduce, 1, 0);
  }
  if (!merged) Push(&st, ChainOp::AllReduceCam);
  if (s.nk) Push(&st, ChainOp::IntrLinearize);
  if (!fin_in_schur && !fin1_in_schur) Push(&st, ChainOp::CamFinalize, merged ? 1 : 0);
  Push(&st, ChainOp::Schur, fin_in_schur ? 1 : (fin1_in_schur ? 2 : 0));
  // S is final after k_S_reduce (tiled Cholesky without border, one rank, no free intrinsics, no merged damping;
  // a forced pack / unpack on one rank is a copy): it also factors the first diagonal tile for k_chol_tiles (zpre),
  // and writes the band a second time, tile-major in the order and layout k_chol_tiles consumes (stile; the forced
  // unpack does not write that copy)
  const int amode = merged ? 2 : (s.assemble ? 1 : 0);
  const bool s_final = s.tiles && !s.border && s.nk == 0 && amode == 1 && !s.multi;
  const bool zpre = s_final && k.chol_zpre;
  st.stile = s_final && !k.pack_force && k.chol_stile;
  Push(&st, ChainOp::SReduce, amode, (zpre ? 1 : 0) | (st.stile ? 2 : 0));
  if (s.nk) Push(&st, ChainOp::IntrSchur);
  if (s.multi || k.pack_force || merged) {
    // the band of S and the rhs partial are summed over landmark shards (packed: the band only), with the merged
    // tail after them
    Push(&st, ChainOp::Exchange, merged, fin1_in_schur);
    if (merged && !fin1_in_schur) Push(&st, ChainOp::CamFinalize, 2);
  }
  Push(&st, ChainOp::Chol, zpre, st.stile);
  if (s.nk) Push(&st, ChainOp::IntrStep);
  // the candidate's camera blocks and linearization scalars beside the update scalars, one launch
  if (k.spec) {
    Push(&st, ChainOp::UpdateLin);
    Push(&st, ChainOp::CamReduce, 2, decide_in_reduce ? 2 : 1);
  } else {
    Push(&st, ChainOp::PointUpdate);
    Push(&st, ChainOp::UpdReduce, s.multi ? 0 : 1);
  }
  if (s.multi) Push(&st, ChainOp::AllReduceUpd);
  if (k.spec)
    st.pending_out = !decide_in_reduce;
  else if (s.multi)
    Push(&st, ChainOp::Decide, 0);
  return st;
}

ChainStep PlanBatchTail(bool pending) {
  ChainStep st;
  if (pending) Push(&st, ChainOp::Decide, 1);
  return st;
}

}  // namespace sg
