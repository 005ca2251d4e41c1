// chain_plan_check.cpp — CPU check of PlanIteration (slam-robot_amd/csrc/ba_chain.cpp): the launches of one LM
// iteration in every regime.  (a) The first iteration and the steady state of the named regimes, written out as
// literal sequences.  (b) Over every combination of knobs and shape, four consecutive iterations: what each step
// must contain whatever the regime (one Schur, reduce and Cholesky; each finalize mode once; a pending decision
// taken first and never dropped; Z_0 and the tile-major copy only when S is final after k_S_reduce; the shards'
// all-reduces).  Built stand-alone with -fsanitize=address,undefined by tests/test_chain_plan.py.
#include <cstdio>
#include <string>

#include "ba_chain.h"

using namespace sg;

static int g_fail = 0;
static std::string g_case;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      if (++g_fail <= 40) printf("FAIL [%s] %s:%d: %s\n", g_case.c_str(), __FILE__, __LINE__, #cond); \
    }                                                                                    \
  } while (0)

static const struct {
  const char* name;
  int nargs;
} kOps[(int)ChainOp::kCount] = {
    {"Linearize", 0}, {"CamReduce", 2}, {"Decide", 1},    {"AllReduceCam", 0}, {"IntrLinearize", 0}, {"CamFinalize", 1},
    {"Schur", 1},     {"SReduce", 2},   {"IntrSchur", 0}, {"Exchange", 2},     {"Chol", 2},          {"IntrStep", 0},
    {"UpdateLin", 0}, {"PointUpdate", 0}, {"UpdReduce", 1}, {"AllReduceUpd", 0}};

static std::string Text(const ChainStep& st) {
  std::string s;
  for (int i = 0; i < st.n; ++i) {
    const ChainCall c = st.ops[i];
    if (i) s += " ";
    s += kOps[(int)c.op].name;
    if (kOps[(int)c.op].nargs == 1) s += "(" + std::to_string(c.a) + ")";
    if (kOps[(int)c.op].nargs == 2) s += "(" + std::to_string(c.a) + "," + std::to_string(c.b) + ")";
  }
  return s;
}

static void Expect(const char* what, const ChainStep& st, const std::string& want, bool pending_out, bool stile) {
  g_case = what;
  const std::string got = Text(st);
  if (got != want) printf("[%s]\n  got  %s\n  want %s\n", what, got.c_str(), want.c_str());
  CHECK(got == want);
  CHECK(st.pending_out == pending_out);
  CHECK(st.stile == stile);
}

// ---- (a) the regimes, as literal sequences (tiled Cholesky, no border, no free intrinsics unless named)
static void CheckSequences() {
  const ChainShape one{false, true, 0, true, false};
  const ChainShape rank0{true, true, 0, true, false}, rank1{true, false, 0, true, false};
  const RunKnobs def;
  Expect("one rank, first", PlanIteration(one, def, true, false),
         "Linearize CamReduce(1,0) AllReduceCam CamFinalize(0) Schur(0) SReduce(1,3) Chol(1,1) UpdateLin CamReduce(2,2)",
         false, true);
  // the five launches of DESIGN.md 4 (the all-reduce is a no-op on one rank)
  Expect("one rank, steady", PlanIteration(one, def, false, false),
         "AllReduceCam Schur(1) SReduce(1,3) Chol(1,1) UpdateLin CamReduce(2,2)", false, true);
  {
    RunKnobs k;
    k.chol_zpre = false;
    Expect("one rank, steady, no zpre", PlanIteration(one, k, false, false),
           "AllReduceCam Schur(1) SReduce(1,2) Chol(0,1) UpdateLin CamReduce(2,2)", false, true);
    k = def;
    k.chol_stile = false;
    Expect("one rank, steady, no stile", PlanIteration(one, k, false, false),
           "AllReduceCam Schur(1) SReduce(1,1) Chol(1,0) UpdateLin CamReduce(2,2)", false, false);
  }
  {
    RunKnobs k;
    k.spec = false;
    const char* want =
        "Linearize CamReduce(1,0) AllReduceCam CamFinalize(0) Schur(0) SReduce(1,3) Chol(1,1) PointUpdate UpdReduce(1)";
    Expect("one rank, two-pass, first", PlanIteration(one, k, true, false), want, false, true);
    Expect("one rank, two-pass, steady", PlanIteration(one, k, false, false), want, false, true);
  }
  {
    const char* want = "Decide(1) Schur(2) SReduce(2,0) Exchange(1,1) Chol(0,0) UpdateLin CamReduce(2,1) AllReduceUpd";
    Expect("two ranks, merged, steady, rank 0", PlanIteration(rank0, def, false, true), want, true, false);
    Expect("two ranks, merged, steady, rank 1", PlanIteration(rank1, def, false, true), want, true, false);
    // a solve's first iteration sums the camera blocks first: the unmerged chain
    Expect("two ranks, first", PlanIteration(rank0, def, true, false),
           "Linearize CamReduce(1,0) AllReduceCam CamFinalize(0) Schur(0) SReduce(1,0) Exchange(0,0) Chol(0,0) UpdateLin "
           "CamReduce(2,1) AllReduceUpd",
           true, false);
  }
  {
    RunKnobs k;
    k.merge = 0;
    Expect("two ranks, unmerged, steady, rank 0", PlanIteration(rank0, k, false, true),
           "Decide(1) AllReduceCam CamFinalize(0) Schur(0) SReduce(1,0) Exchange(0,0) Chol(0,0) UpdateLin CamReduce(2,1) "
           "AllReduceUpd",
           true, false);
    Expect("two ranks, unmerged, steady, rank 1", PlanIteration(rank1, k, false, true),
           "Decide(1) AllReduceCam CamFinalize(0) Schur(0) SReduce(0,0) Exchange(0,0) Chol(0,0) UpdateLin CamReduce(2,1) "
           "AllReduceUpd",
           true, false);
    k.spec = false;
    Expect("two ranks, unmerged, two-pass", PlanIteration(rank0, k, false, false),
           "Linearize CamReduce(1,0) AllReduceCam CamFinalize(0) Schur(0) SReduce(1,0) Exchange(0,0) Chol(0,0) PointUpdate "
           "UpdReduce(0) AllReduceUpd Decide(0)",
           false, false);
  }
  {
    RunKnobs k;
    k.merge = 2;
    Expect("one rank, forced merge, first", PlanIteration(one, k, true, false),
           "Linearize CamReduce(1,0) AllReduceCam CamFinalize(0) Schur(0) SReduce(1,3) Chol(1,1) UpdateLin CamReduce(2,1)",
           true, true);
    Expect("one rank, forced merge, steady", PlanIteration(one, k, false, true),
           "Decide(1) Schur(2) SReduce(2,0) Exchange(1,1) Chol(0,0) UpdateLin CamReduce(2,1)", true, false);
    k.spec = false;
    Expect("one rank, forced merge, two-pass, steady", PlanIteration(one, k, false, false),
           "Linearize CamReduce(1,0) CamFinalize(1) Schur(0) SReduce(2,0) Exchange(1,0) CamFinalize(2) Chol(0,0) "
           "PointUpdate UpdReduce(1)",
           false, false);
  }
  {
    const ChainShape intr{false, true, 7, true, true};
    Expect("free intrinsics, steady", PlanIteration(intr, def, false, true),
           "Decide(1) AllReduceCam IntrLinearize CamFinalize(0) Schur(0) SReduce(1,0) IntrSchur Chol(0,0) IntrStep "
           "UpdateLin CamReduce(2,1)",
           true, false);
  }
  {
    RunKnobs k;
    k.pack_force = true;   // the forced exchange is a copy: Z_0 stays, the tile-major copy does not
    Expect("one rank, forced pack, steady", PlanIteration(one, k, false, false),
           "AllReduceCam Schur(1) SReduce(1,1) Exchange(0,0) Chol(1,0) UpdateLin CamReduce(2,2)", false, false);
  }
  Expect("batch tail, pending", PlanBatchTail(true), "Decide(1)", false, false);
  Expect("batch tail, nothing pending", PlanBatchTail(false), "", false, false);
}

// ---- (b) what every step keeps
static int Count(const ChainStep& st, ChainOp op, int a = -1, int b = -1) {
  int n = 0;
  for (int i = 0; i < st.n; ++i)
    n += st.ops[i].op == op && (a < 0 || st.ops[i].a == a) && (b < 0 || st.ops[i].b == b);
  return n;
}
static int First(const ChainStep& st, ChainOp op) {
  for (int i = 0; i < st.n; ++i)
    if (st.ops[i].op == op) return i;
  return -1;
}

static void CheckStep(const ChainShape& s, const RunKnobs& k, bool first_it, bool pending_in, const ChainStep& st) {
  CHECK(st.n <= kChainMaxOps);
  for (int i = 0; i < st.n; ++i) CHECK((int)st.ops[i].op >= 0 && st.ops[i].op < ChainOp::kCount);
  const bool merged = !first_it && s.nk == 0 && (k.merge == 2 || (s.multi && k.merge == 1));
  // one Schur, one reduce of S, one Cholesky; one point pass and one closing reduce, of the same chain
  CHECK(Count(st, ChainOp::Schur) == 1 && Count(st, ChainOp::SReduce) == 1 && Count(st, ChainOp::Chol) == 1);
  CHECK(Count(st, ChainOp::UpdateLin) + Count(st, ChainOp::PointUpdate) == 1);
  CHECK(Count(st, ChainOp::CamReduce, 2) + Count(st, ChainOp::UpdReduce) == 1);
  CHECK(Count(st, ChainOp::UpdateLin) == (k.spec ? 1 : 0) && Count(st, ChainOp::CamReduce, 2) == (k.spec ? 1 : 0));
  CHECK(st.ops[First(st, ChainOp::Schur)].a >= 0 && st.ops[First(st, ChainOp::Schur)].a <= 2);
  // each mode of the finalize pass exactly once
  const int fin0 = Count(st, ChainOp::CamFinalize, 0) + Count(st, ChainOp::Schur, 1);
  const int fin1 = Count(st, ChainOp::CamFinalize, 1) + Count(st, ChainOp::Schur, 2);
  const int fin2 = Count(st, ChainOp::CamFinalize, 2) + Count(st, ChainOp::Exchange, -1, 1);
  CHECK(fin0 == (merged ? 0 : 1) && fin1 == (merged ? 1 : 0) && fin2 == (merged ? 1 : 0));
  CHECK(Count(st, ChainOp::CamFinalize) + Count(st, ChainOp::Schur, 1) + Count(st, ChainOp::Schur, 2) +
            Count(st, ChainOp::Exchange, -1, 1) == fin0 + fin1 + fin2);
  CHECK((Count(st, ChainOp::SReduce, 2) == 1) == merged);
  // mode 1 before the Schur launch's segments end, mode 2 after the exchange and before the Cholesky
  if (Count(st, ChainOp::CamFinalize, 2))
    CHECK(First(st, ChainOp::Exchange) >= 0 && st.ops[First(st, ChainOp::Exchange) + 1].op == ChainOp::CamFinalize &&
          st.ops[First(st, ChainOp::Exchange) + 1].a == 2);
  // a pending decision is taken before anything else, and only a pending one
  CHECK(Count(st, ChainOp::Decide, 1) == (pending_in ? 1 : 0));
  if (pending_in) CHECK(First(st, ChainOp::Decide) == 0 && st.ops[0].a == 1 && First(st, ChainOp::Schur) > 0);
  if (!k.spec) CHECK(!st.pending_out);
  CHECK(st.pending_out == (Count(st, ChainOp::CamReduce, 2, 1) == 1));
  CHECK(Count(st, ChainOp::CamReduce, 2, 1) + Count(st, ChainOp::CamReduce, 2, 2) == Count(st, ChainOp::CamReduce, 2));
  // the two-pass chain decides in its closing reduce, or on shards after the scalars' all-reduce
  if (!k.spec) CHECK(Count(st, ChainOp::UpdReduce, 1) + Count(st, ChainOp::Decide, 0) == 1);
  if (k.spec) CHECK(Count(st, ChainOp::Decide, 0) == 0);
  if (Count(st, ChainOp::Decide, 0)) CHECK(st.ops[st.n - 1].op == ChainOp::Decide && st.ops[st.n - 2].op == ChainOp::AllReduceUpd);
  // k_linearize and the opening camera reduce: the two-pass chain, or a solve's first iteration
  CHECK(Count(st, ChainOp::Linearize) == ((!k.spec || first_it) ? 1 : 0));
  CHECK(Count(st, ChainOp::CamReduce, 1, 0) == Count(st, ChainOp::Linearize));
  CHECK(Count(st, ChainOp::CamReduce) == Count(st, ChainOp::CamReduce, 1, 0) + Count(st, ChainOp::CamReduce, 2));
  // Z_0 and the tile-major copy: only when S is final after k_S_reduce
  const ChainCall sr = st.ops[First(st, ChainOp::SReduce)], ch = st.ops[First(st, ChainOp::Chol)];
  const bool zpre = sr.b & 1, stile = sr.b & 2;
  CHECK(sr.b >= 0 && sr.b <= 3 && ch.a == (zpre ? 1 : 0) && ch.b == (stile ? 1 : 0) && st.stile == stile);
  CHECK(sr.a == (merged ? 2 : s.assemble ? 1 : 0));
  const int nx = Count(st, ChainOp::Exchange);
  const bool s_final = s.tiles && !s.border && s.nk == 0 && sr.a == 1 && (nx == 0 || (!s.multi && k.pack_force));
  CHECK(zpre == (s_final && k.chol_zpre));
  CHECK(stile == (s_final && nx == 0 && k.chol_stile));
  if (stile) CHECK(nx == 0);
  // the free intrinsics' launches
  for (ChainOp op : {ChainOp::IntrLinearize, ChainOp::IntrSchur, ChainOp::IntrStep}) CHECK(Count(st, op) == (s.nk > 0 ? 1 : 0));
  // the exchanges
  CHECK(nx == ((s.multi || k.pack_force || merged) ? 1 : 0));
  CHECK(Count(st, ChainOp::Exchange, 1) == ((nx && merged) ? 1 : 0));
  const int nar = Count(st, ChainOp::AllReduceCam) + nx + Count(st, ChainOp::AllReduceUpd);
  if (s.multi) CHECK(nar == (merged ? 2 : 3));
  CHECK(Count(st, ChainOp::AllReduceUpd) == (s.multi ? 1 : 0));
  CHECK(Count(st, ChainOp::AllReduceCam) == (merged ? 0 : 1));
  // order: Schur, the reduce of S, the exchange, the Cholesky, the point pass, the closing reduce
  CHECK(First(st, ChainOp::Schur) < First(st, ChainOp::SReduce) && First(st, ChainOp::SReduce) < First(st, ChainOp::Chol));
  if (nx) CHECK(First(st, ChainOp::SReduce) < First(st, ChainOp::Exchange) && First(st, ChainOp::Exchange) < First(st, ChainOp::Chol));
  // (the driver passes 0 for k_cam_finalize's decide argument: no op carries one.  CamFinalize has its mode only.)
  for (int i = 0; i < st.n; ++i)
    if (st.ops[i].op == ChainOp::CamFinalize) CHECK(st.ops[i].b == 0);
}

static void CheckInvariants() {
  long steps = 0;
  for (int bits = 0; bits < (1 << 11); ++bits)
    for (int merge = 0; merge < 3; ++merge) {
      RunKnobs k;
      ChainShape s;
      k.spec = bits & 1;
      k.merge = merge;
      k.pack_force = bits & 2;
      k.chol_zpre = bits & 4;
      k.chol_stile = bits & 8;
      s.multi = bits & 16;
      s.assemble = bits & 32;
      s.nk = (bits & 64) ? 7 : 0;
      s.tiles = bits & 128;
      s.border = bits & 256;
      bool first_it = bits & 512, pending = bits & 1024;
      char buf[160];
      for (int it = 0; it < 4; ++it) {
        snprintf(buf, sizeof(buf), "spec %d merge %d pack %d zpre %d stile %d multi %d assemble %d nk %d tiles %d border %d "
                 "first %d pending %d it %d", k.spec, k.merge, k.pack_force, k.chol_zpre, k.chol_stile, s.multi, s.assemble,
                 s.nk, s.tiles, s.border, (int)first_it, (int)pending, it);
        g_case = buf;
        const ChainStep st = PlanIteration(s, k, first_it, pending);
        CheckStep(s, k, first_it, pending, st);
        first_it = false;
        pending = st.pending_out;
        ++steps;
      }
      const ChainStep tail = PlanBatchTail(pending);
      CHECK(tail.n == (pending ? 1 : 0) && !tail.pending_out);
      if (pending) CHECK(tail.ops[0].op == ChainOp::Decide && tail.ops[0].a == 1);
    }
  printf("%ld steps checked\n", steps);
}

int main() {
  CheckSequences();
  CheckInvariants();
  if (g_fail) {
    printf("chain_plan_check FAILED (%d)\n", g_fail);
    return 1;
  }
  printf("chain_plan_check OK\n");
  return 0;
}
