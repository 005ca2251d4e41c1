// posegraph_plan_check.cpp — CPU check of csrc/posegraph_plan.cpp, a stand-alone program (tests/test_posegraph_plan.py
// builds it twice, once under AddressSanitizer and UBSan).  On seeded random graphs (fixed nodes, duplicate edges,
// several graphs per call): the elimination order is a greedy minimum-degree order with ties to the lower list
// position; L's pattern equals a dense boolean elimination in that order; every assembly contribution and every
// update triple is present exactly once, in listed edge order, and a target appears at most once per column; the
// status rules, on a graph of two components of which one has no fixed node; every SG_EINVAL of the contract, the size
// caps included.  With a case file (chords24 from tests/posegraph_cases.py): the CPU executor's solve of the first
// linearization against a dense Cholesky solve of the same system, to the tolerances the file carries.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "common.h"
#include "posegraph_plan.h"

using namespace sg;

namespace sg {
void SetError(const std::string&) {}
}  // namespace sg

static int g_fail = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      ++g_fail;                                \
    }                                          \
  } while (0)

struct Call {
  std::vector<double> q, t;
  std::vector<int32_t> frame, fixed, noff{0}, ab, eoff{0};
  std::vector<double> meas, w;
  sg_posegraph_options o{0.0, 0, 0};
  sg_map Map() {
    sg_map m{};
    m.num_frames = (int32_t)(q.size() / 4);
    m.q = q.data();
    m.t = t.data();
    return m;
  }
  int n() const { return (int)noff.size() - 1; }
  void AddGraph(int nn, const std::vector<int>& fx, const std::vector<std::pair<int, int>>& edges) {
    const int f0 = (int)frame.size();
    for (int i = 0; i < nn; ++i) {
      frame.push_back(f0 + i);
      fixed.push_back(fx[i]);
      const double qi[4] = {0, 0, 0, 1};
      q.insert(q.end(), qi, qi + 4);
      for (int k = 0; k < 3; ++k) t.push_back(10.0 * (f0 + i) + k);
    }
    for (auto& e : edges) {
      ab.push_back(e.first);
      ab.push_back(e.second);
      const double mm[8] = {0, 0, 0, 1, 1, 2, 3, 0};
      meas.insert(meas.end(), mm, mm + 8);
      const double ww[3] = {1, 1, 1};
      w.insert(w.end(), ww, ww + 3);
    }
    noff.push_back((int32_t)frame.size());
    eoff.push_back((int32_t)(ab.size() / 2));
  }
  int Plan(PgPlan* pl) {
    sg_map m = Map();
    try {
      PlanPoseGraph(&m, frame.data(), fixed.data(), noff.data(), ab.data(), meas.data(), w.data(), eoff.data(), n(), &o,
                    pl);
    } catch (const Error& e) {
      return e.code;
    }
    return 0;
  }
};

static void CheckGraph(const Call& c, const PgPlan& pl, int g) {
  const PgGraph& G = pl.graphs[g];
  const int32_t* fixed = c.fixed.data() + G.node0;
  const int32_t* ab = c.ab.data() + 2 * (size_t)G.edge0;
  CHECK(G.node0 == c.noff[g] && G.nn == c.noff[g + 1] - c.noff[g] && G.edge0 == c.eoff[g] &&
            G.ne == c.eoff[g + 1] - c.eoff[g], "graph %d: ranges", g);
  // status by brute force
  int nfree = 0;
  bool touched = false;
  for (int i = 0; i < G.nn; ++i) nfree += !fixed[i];
  for (int e = 0; e < G.ne; ++e) touched |= !fixed[ab[2 * e]] || !fixed[ab[2 * e + 1]];
  int want = SG_PG_OK;
  if (!nfree || !touched) {
    want = SG_PG_DID_NOT_RUN;
  } else {
    std::vector<int> comp((size_t)G.nn);
    for (int i = 0; i < G.nn; ++i) comp[i] = i;
    for (bool ch = true; ch;) {
      ch = false;
      for (int e = 0; e < G.ne; ++e) {
        const int lo = std::min(comp[ab[2 * e]], comp[ab[2 * e + 1]]);
        if (comp[ab[2 * e]] != lo || comp[ab[2 * e + 1]] != lo) ch = true;
        comp[ab[2 * e]] = comp[ab[2 * e + 1]] = lo;
      }
    }
    for (int i = 0; i < G.nn; ++i) {
      if (fixed[i]) continue;
      bool anchored = false;
      for (int k = 0; k < G.nn; ++k) anchored |= fixed[k] && comp[k] == comp[i];
      if (!anchored) want = SG_PG_NO_ANCHOR;
    }
  }
  CHECK(G.status == want && G.run == (want == SG_PG_OK), "graph %d: status %d, expected %d", g, G.status, want);
  if (!G.run) {
    CHECK(G.nc == 0 && G.nb == 0, "graph %d: a graph that does not run has columns", g);
    return;
  }
  CHECK(G.nc == nfree, "graph %d: %d columns for %d free nodes", g, G.nc, nfree);
  // the order is a permutation of the free nodes, and greedy minimum degree with ties to the lower list position
  std::vector<int> col((size_t)G.nn, -1);
  for (int j = 0; j < G.nc; ++j) {
    const int nd = pl.col_node[G.col0 + j];
    CHECK(nd >= 0 && nd < G.nn && !fixed[nd] && col[nd] < 0, "graph %d: column %d's node", g, j);
    col[nd] = j;
  }
  for (int i = 0; i < G.nn; ++i) CHECK(pl.node_col[G.node0 + i] == col[i], "graph %d: node_col[%d]", g, i);
  std::vector<std::vector<uint8_t>> A((size_t)G.nn, std::vector<uint8_t>((size_t)G.nn, 0));
  for (int e = 0; e < G.ne; ++e)
    if (!fixed[ab[2 * e]] && !fixed[ab[2 * e + 1]]) A[ab[2 * e]][ab[2 * e + 1]] = A[ab[2 * e + 1]][ab[2 * e]] = 1;
  std::vector<uint8_t> gone((size_t)G.nn, 0);
  std::set<std::pair<int, int>> pattern;   // (column, row), row > column, of the dense boolean elimination
  for (int j = 0; j < G.nc; ++j) {
    const int v = pl.col_node[G.col0 + j];
    auto deg = [&](int i) {
      int d = 0;
      for (int k = 0; k < G.nn; ++k) d += !gone[k] && !fixed[k] && k != i && A[i][k];
      return d;
    };
    const int dv = deg(v);
    for (int i = 0; i < G.nn; ++i) {
      if (fixed[i] || gone[i] || i == v) continue;
      const int di = deg(i);
      CHECK(di > dv || (di == dv && i > v), "graph %d: column %d is node %d (degree %d), node %d has %d", g, j, v, dv, i,
            di);
    }
    gone[v] = 1;
    std::vector<int> nb;
    for (int k = 0; k < G.nn; ++k)
      if (!gone[k] && !fixed[k] && A[v][k]) nb.push_back(k);
    for (int a : nb)
      for (int b : nb)
        if (a != b) A[a][b] = 1;
    for (int a : nb) pattern.insert({j, -1 - a});   // rows by node for now (their columns are not all known yet)
  }
  std::set<std::pair<int, int>> want_pat;
  for (auto& p : pattern) want_pat.insert({p.first, col[-1 - p.second]});
  std::map<std::pair<int, int>, int> block;   // (row, column) -> call-wide block
  std::set<std::pair<int, int>> got_pat;
  for (int j = 0; j < G.nc; ++j) {
    const int b0 = pl.colptr[G.col0 + j], b1 = pl.colptr[G.col0 + j + 1];
    CHECK(b1 > b0 && pl.blk_row[b0] == j, "graph %d: column %d does not start with its diagonal block", g, j);
    for (int B = b0; B < b1; ++B) {
      CHECK(pl.blk_col[B] == j, "graph %d: blk_col", g);
      CHECK(B == b0 || pl.blk_row[B] > pl.blk_row[B - 1], "graph %d: column %d's rows do not ascend", g, j);
      block[{pl.blk_row[B], j}] = B;
      if (B > b0) got_pat.insert({j, pl.blk_row[B]});
    }
  }
  CHECK(got_pat == want_pat, "graph %d: fill differs from the dense elimination (%zu vs %zu blocks)", g, got_pat.size(),
        want_pat.size());
  CHECK(pl.colptr[G.col0] == G.blk0 && pl.colptr[G.col0 + G.nc] == G.blk0 + G.nb, "graph %d: block range", g);
  // assembly lists: every contribution exactly once, in listed edge order
  std::map<int, std::vector<int>> want_asm, want_g;
  for (int e = 0; e < G.ne; ++e) {
    const int ca = col[ab[2 * e]], cb = col[ab[2 * e + 1]];
    if (ca >= 0) {
      want_asm[block[{ca, ca}]].push_back(4 * e);
      want_g[ca].push_back(2 * e);
    }
    if (cb >= 0) {
      want_asm[block[{cb, cb}]].push_back(4 * e + 1);
      want_g[cb].push_back(2 * e + 1);
    }
    if (ca >= 0 && cb >= 0) want_asm[block[{std::max(ca, cb), std::min(ca, cb)}]].push_back(4 * e + (ca > cb ? 2 : 3));
  }
  for (int B = G.blk0; B < G.blk0 + G.nb; ++B) {
    std::vector<int> got(pl.asm_items.begin() + pl.asm_ptr[B], pl.asm_items.begin() + pl.asm_ptr[B + 1]);
    CHECK(got == want_asm[B], "graph %d: assembly list of block %d", g, B);
  }
  for (int j = 0; j < G.nc; ++j) {
    std::vector<int> got(pl.gasm_items.begin() + pl.gasm_ptr[G.col0 + j], pl.gasm_items.begin() + pl.gasm_ptr[G.col0 + j + 1]);
    CHECK(got == want_g[j], "graph %d: gradient list of column %d", g, j);
  }
  // update lists: for every pair of rows i >= k of column j the triple once, and no target twice in a column
  for (int j = 0; j < G.nc; ++j) {
    const int b0 = pl.colptr[G.col0 + j], b1 = pl.colptr[G.col0 + j + 1];
    std::set<std::pair<int, int>> want_u, got_u;
    for (int p = b0 + 1; p < b1; ++p)
      for (int q = p; q < b1; ++q) want_u.insert({q, p});
    std::set<int> targets;
    for (int u = pl.upd_ptr[G.col0 + j]; u < pl.upd_ptr[G.col0 + j + 1]; ++u) {
      const int Bi = pl.upd[3 * u], Bk = pl.upd[3 * u + 1], T = pl.upd[3 * u + 2];
      CHECK(got_u.insert({Bi, Bk}).second, "graph %d: column %d lists a triple twice", g, j);
      CHECK(targets.insert(T).second, "graph %d: column %d updates block %d twice", g, j, T);
      CHECK(T >= G.blk0 && T < G.blk0 + G.nb && pl.blk_row[T] == pl.blk_row[Bi] && pl.blk_col[T] == pl.blk_row[Bk],
            "graph %d: column %d's target", g, j);
    }
    CHECK(got_u == want_u, "graph %d: update list of column %d", g, j);
  }
}

static void RandomCalls() {
  std::mt19937 rng(11);
  for (int rep = 0; rep < 40; ++rep) {
    Call c;
    const int ng = 1 + rng() % 3;
    for (int g = 0; g < ng; ++g) {
      const int nn = 1 + rng() % 30;
      std::vector<int> fx((size_t)nn);
      for (int& f : fx) f = rng() % 5 == 0;
      std::vector<std::pair<int, int>> ed;
      const int ne = nn < 2 ? 0 : (int)(rng() % (3 * nn));
      for (int e = 0; e < ne; ++e) {
        const int a = rng() % nn;
        int b = rng() % nn;
        if (b == a) b = (a + 1) % nn;
        ed.push_back({a, b});
      }
      c.AddGraph(nn, fx, ed);
    }
    PgPlan pl;
    CHECK(c.Plan(&pl) == 0, "random call %d refused", rep);
    if ((int)pl.graphs.size() != c.n()) continue;
    for (int g = 0; g < c.n(); ++g) CheckGraph(c, pl, g);
    CHECK(pl.asm_ptr.size() == pl.blk_row.size() + 1 && pl.colptr.size() == pl.col_node.size() + 1 &&
              pl.upd_ptr.size() == pl.col_node.size() + 1 && pl.gasm_ptr.size() == pl.col_node.size() + 1,
          "call %d: list sizes", rep);
  }
}

static void StatusRules() {
  Call c;
  // two components: a ring of 6 with node 0 fixed, a ring of 5 with no fixed node
  std::vector<std::pair<int, int>> ed;
  for (int i = 0; i < 6; ++i) ed.push_back({i, (i + 1) % 6});
  for (int i = 0; i < 5; ++i) ed.push_back({6 + i, 6 + (i + 1) % 5});
  std::vector<int> fx(11, 0);
  fx[0] = 1;
  c.AddGraph(11, fx, ed);
  c.AddGraph(3, {1, 1, 1}, {{0, 1}, {1, 2}});     // no free node
  c.AddGraph(3, {1, 1, 0}, {{0, 1}});             // a free node, but no edge touches one
  c.AddGraph(3, {1, 0, 0}, {{0, 1}});             // node 2 is free and alone
  c.AddGraph(3, {1, 0, 0}, {{0, 1}, {2, 1}});     // anchored through node 1
  c.AddGraph(0, {}, {});                          // empty
  PgPlan pl;
  CHECK(c.Plan(&pl) == 0, "status call refused");
  const int want[6] = {SG_PG_NO_ANCHOR, SG_PG_DID_NOT_RUN, SG_PG_DID_NOT_RUN, SG_PG_NO_ANCHOR, SG_PG_OK, SG_PG_DID_NOT_RUN};
  for (int g = 0; g < 6; ++g) {
    CHECK(pl.graphs[g].status == want[g], "status of graph %d: %d", g, pl.graphs[g].status);
    CheckGraph(c, pl, g);
  }
  CHECK(pl.num_run == 1, "num_run %d", pl.num_run);
}

static void ArgumentErrors() {
  auto base = [] {
    Call c;
    c.AddGraph(4, {1, 0, 0, 0}, {{0, 1}, {1, 2}, {2, 3}});
    return c;
  };
  PgPlan pl;
  {
    Call c = base();
    CHECK(c.Plan(&pl) == 0, "base call refused");
    sg_map m = c.Map();
    auto call = [&](const sg_map* mp, const int32_t* fr, const int32_t* fx, const int32_t* no, const int32_t* ab,
                    const double* me, const double* w, const int32_t* eo, int n, const sg_posegraph_options* o) {
      try {
        PlanPoseGraph(mp, fr, fx, no, ab, me, w, eo, n, o, &pl);
      } catch (const Error& e) {
        return e.code;
      }
      return 0;
    };
    auto F = c.frame.data();
    auto X = c.fixed.data();
    auto N = c.noff.data();
    auto A = c.ab.data();
    auto M = c.meas.data();
    auto W = c.w.data();
    auto E = c.eoff.data();
    CHECK(call(nullptr, F, X, N, A, M, W, E, 1, &c.o) == SG_EINVAL, "null map");
    CHECK(call(&m, F, X, N, A, M, W, E, 1, nullptr) == SG_EINVAL, "null options");
    CHECK(call(&m, F, X, N, A, M, W, E, -1, &c.o) == SG_EINVAL, "negative n");
    CHECK(call(&m, nullptr, X, N, A, M, W, E, 1, &c.o) == SG_EINVAL, "null node_frame");
    CHECK(call(&m, F, nullptr, N, A, M, W, E, 1, &c.o) == SG_EINVAL, "null node_fixed");
    CHECK(call(&m, F, X, nullptr, A, M, W, E, 1, &c.o) == SG_EINVAL, "null node_offset");
    CHECK(call(&m, F, X, N, nullptr, M, W, E, 1, &c.o) == SG_EINVAL, "null edge_ab");
    CHECK(call(&m, F, X, N, A, nullptr, W, E, 1, &c.o) == SG_EINVAL, "null edge_meas");
    CHECK(call(&m, F, X, N, A, M, nullptr, E, 1, &c.o) == SG_EINVAL, "null edge_weight");
    CHECK(call(&m, F, X, N, A, M, W, nullptr, 1, &c.o) == SG_EINVAL, "null edge_offset");
    CHECK(call(&m, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &c.o) == 0, "n == 0 with null lists");
    sg_map m2 = m;
    m2.q = nullptr;
    CHECK(call(&m2, F, X, N, A, M, W, E, 1, &c.o) == SG_EINVAL, "map without poses");
    for (double r : {-1.0, (double)NAN, (double)INFINITY}) {
      sg_posegraph_options o = c.o;
      o.range = r;
      CHECK(call(&m, F, X, N, A, M, W, E, 1, &o) == SG_EINVAL, "range %g", r);
    }
    sg_posegraph_options mv = c.o;
    mv.move_points = 1;
    CHECK(call(&m, F, X, N, A, M, W, E, 1, &mv) == 0, "move_points on a map without observations");
    m2 = m;
    m2.num_obs = 3;
    CHECK(call(&m2, F, X, N, A, M, W, E, 1, &mv) == SG_EINVAL, "move_points on a map whose observations cannot be read");
  }
  auto refused = [&](const char* what, Call c) { CHECK(c.Plan(&pl) == SG_EINVAL, "%s accepted", what); };
  { Call c = base(); c.noff[0] = 1; refused("node_offset[0] != 0", c); }
  { Call c = base(); c.eoff[0] = 1; refused("edge_offset[0] != 0", c); }
  { Call c = base(); c.AddGraph(2, {1, 0}, {{0, 1}}); c.noff[1] = 6; c.noff[2] = 5; refused("decreasing node offset", c); }
  { Call c = base(); c.AddGraph(2, {1, 0}, {{0, 1}}); c.eoff[1] = 4; c.eoff[2] = 3; refused("decreasing edge offset", c); }
  for (int bad : {-1, 4, 1 << 30}) { Call c = base(); c.frame[2] = bad; refused("frame index out of range", c); }
  { Call c = base(); c.frame[2] = c.frame[1]; refused("frame listed twice", c); }
  { Call c = base(); c.AddGraph(2, {1, 0}, {{0, 1}}); c.frame[5] = 0; refused("frame listed in two graphs", c); }
  for (int bad : {-1, 4}) { Call c = base(); c.ab[3] = bad; refused("edge index out of range", c); }
  { Call c = base(); c.ab[2] = c.ab[3]; refused("a == b", c); }
  for (double bad : {0.0, 1.001, (double)NAN}) { Call c = base(); c.meas[8 + 3] = bad; refused("q^ not unit", c); }
  for (int k : {4, 7}) { Call c = base(); c.meas[8 + k] = INFINITY; refused("u^ or rho^ not finite", c); }
  for (double bad : {0.0, -1.0, (double)NAN, (double)INFINITY})
    for (int k = 0; k < 3; ++k) { Call c = base(); c.w[3 + k] = bad; refused("bad weight", c); }
  { Call c = base(); c.w[5] = -1.0; c.o.fix_scale = 1; CHECK(c.Plan(&pl) == 0, "w_s is read with fix_scale"); }
  // caps: nodes and edges per graph, and the blocks of a call (128 complete graphs of 46 free nodes: 1081 blocks each)
  {
    Call c;
    std::vector<int> fx((size_t)kPgMaxNodes + 1, 0);
    fx[0] = 1;
    std::vector<std::pair<int, int>> ed;
    for (int i = 0; i < kPgMaxNodes; ++i) ed.push_back({i, i + 1});
    c.AddGraph(kPgMaxNodes + 1, fx, ed);
    refused("too many nodes in a graph", c);
  }
  {
    Call c;
    std::vector<std::pair<int, int>> ed((size_t)kPgMaxEdges + 1, {0, 1});
    c.AddGraph(2, {1, 0}, ed);
    refused("too many edges in a graph", c);
    Call d;
    ed.pop_back();
    d.AddGraph(2, {1, 0}, ed);
    CHECK(d.Plan(&pl) == 0, "kPgMaxEdges edges refused");
  }
  {
    // the call's caps on the factors: grids of 32 x 32 nodes fill in; as many as fit are accepted, one more is not
    const int S = 32;
    std::vector<std::pair<int, int>> ed;
    for (int r = 0; r < S; ++r)
      for (int k = 0; k < S; ++k) {
        if (k + 1 < S) ed.push_back({r * S + k, r * S + k + 1});
        if (r + 1 < S) ed.push_back({r * S + k, (r + 1) * S + k});
      }
    std::vector<int> fx((size_t)S * S, 0);
    fx[0] = 1;
    Call one;
    one.AddGraph(S * S, fx, ed);
    CHECK(one.Plan(&pl) == 0, "one grid refused");
    const int nb1 = (int)pl.blk_row.size(), nu1 = (int)(pl.upd.size() / 3);
    const int fit = std::min(kPgMaxCallBlocks / nb1, kPgMaxCallUpdates / nu1);
    std::printf("grid %d x %d: %d blocks, %d updates; %d grids fit a call\n", S, S, nb1, nu1, fit);
    CHECK((size_t)(fit + 1) * ed.size() <= (size_t)kPgMaxCallEdges, "the edge cap comes before the factor caps");
    Call c;
    for (int g = 0; g < fit; ++g) c.AddGraph(S * S, fx, ed);
    CHECK(c.Plan(&pl) == 0, "%d grids refused", fit);
    c.AddGraph(S * S, fx, ed);
    refused("a call over the factor caps", c);
    Call e;
    for (int g = 0; g * 2 <= kPgMaxCallEdges + 1; ++g) e.AddGraph(2, {1, 0}, {{0, 1}, {1, 0}});
    refused("too many edges in a call", e);
    Call f;
    for (int g = 0; g * 1024 <= kPgMaxCallNodes; ++g) f.AddGraph(1024, std::vector<int>(1024, 1), {});
    refused("too many nodes in a call", f);
  }
}

// The executor against a dense solve on one linearization of a case file: N, E, D-free poses, flags, edges, then the
// tolerances on the step (rotation rad, centre, log-scale).
static void ExecutorAgainstDense(const char* path) {
  std::ifstream in(path);
  int N, E;
  in >> N >> E;
  Call c;
  c.q.resize(4 * (size_t)N);
  c.t.resize(3 * (size_t)N);
  c.fixed.resize((size_t)N);
  for (int i = 0; i < N; ++i) {
    for (int k = 0; k < 4; ++k) in >> c.q[4 * i + k];
    for (int k = 0; k < 3; ++k) in >> c.t[3 * i + k];
    in >> c.fixed[i];
    c.frame.push_back(i);
  }
  c.ab.resize(2 * (size_t)E);
  c.meas.resize(8 * (size_t)E);
  c.w.resize(3 * (size_t)E);
  for (int e = 0; e < E; ++e) {
    in >> c.ab[2 * e] >> c.ab[2 * e + 1];
    for (int k = 0; k < 8; ++k) in >> c.meas[8 * e + k];
    for (int k = 0; k < 3; ++k) in >> c.w[3 * e + k];
  }
  double tol[3], radius;
  in >> tol[0] >> tol[1] >> tol[2] >> radius;
  CHECK((bool)in, "case file %s is short", path);
  c.noff.push_back(N);
  c.eoff.push_back(E);
  PgPlan pl;
  CHECK(c.Plan(&pl) == 0, "case refused");
  if (pl.graphs.empty() || !pl.graphs[0].run) return;
  CheckGraph(c, pl, 0);
  const PgGraph& G = pl.graphs[0];
  std::vector<double> ws(pl.WorkspaceDoubles(), 0.0);
  const PgView v = pl.View(ws.data());
  const int D = v.D, n = G.nc * D;
  for (int e = 0; e < E; ++e) {
    bool fx;
    PgEdgeLinearize(v, G, e, 0, &fx);
  }
  for (int i = 0; i < n; ++i) PgGradEntry(v, G, i, 0);
  for (int i = 0; i < n; ++i) {
    const size_t a = 7 * (size_t)(i / D) + i % D;
    v.scale[a] = 1.0 / (1.0 + std::sqrt(v.hd[a]));
    v.diag[a] = std::fmin(std::fmax(v.scale[a] * v.scale[a] * v.hd[a], 1e-6), 1e32);
    v.y[a] = v.g[a] * v.scale[a];
  }
  for (int i = 0; i < G.nb * D * D; ++i) PgAssembleEntry(v, G, i, 0, radius);
  // the same system, dense, from the edge records (long double accumulation, plain Cholesky)
  std::vector<long double> H((size_t)n * n, 0.0L), y((size_t)n);
  for (int e = 0; e < E; ++e) {
    const double* J = v.rec[0] + (size_t)kPgRec * e + kPgRes;
    const int cs[2] = {pl.node_col[c.ab[2 * e]], pl.node_col[c.ab[2 * e + 1]]};
    for (int sa = 0; sa < 2; ++sa)
      for (int sb = 0; sb < 2; ++sb) {
        if (cs[sa] < 0 || cs[sb] < 0) continue;
        for (int r = 0; r < D; ++r)
          for (int k = 0; k < D; ++k) {
            long double s = 0.0L;
            for (int q = 0; q < kPgRes; ++q) s += (long double)J[q * kPgCols + 7 * sa + r] * J[q * kPgCols + 7 * sb + k];
            H[(size_t)(cs[sa] * D + r) * n + cs[sb] * D + k] += s;
          }
      }
  }
  for (int i = 0; i < n; ++i) {
    const size_t a = 7 * (size_t)(i / D) + i % D;
    for (int k = 0; k < n; ++k) H[(size_t)i * n + k] *= (long double)v.scale[a] * v.scale[7 * (size_t)(k / D) + k % D];
    H[(size_t)i * n + i] += (long double)v.diag[a] / radius;
    y[i] = v.y[a];
  }
  for (int j = 0; j < n; ++j) {
    for (int k = 0; k < j; ++k) H[(size_t)j * n + j] -= H[(size_t)j * n + k] * H[(size_t)j * n + k];
    H[(size_t)j * n + j] = std::sqrt(H[(size_t)j * n + j]);
    for (int i = j + 1; i < n; ++i) {
      for (int k = 0; k < j; ++k) H[(size_t)i * n + j] -= H[(size_t)i * n + k] * H[(size_t)j * n + k];
      H[(size_t)i * n + j] /= H[(size_t)j * n + j];
    }
  }
  for (int i = 0; i < n; ++i) {
    for (int k = 0; k < i; ++k) y[i] -= H[(size_t)i * n + k] * y[k];
    y[i] /= H[(size_t)i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    for (int k = i + 1; k < n; ++k) y[i] -= H[(size_t)k * n + i] * y[k];
    y[i] /= H[(size_t)i * n + i];
  }
  CHECK(PgCpuFactorSolve(v, G), "the executor met a non-positive pivot");
  double worst[3] = {0, 0, 0};
  for (int i = 0; i < n; ++i) {
    const size_t a = 7 * (size_t)(i / D) + i % D;
    const int kind = i % D < 3 ? 0 : i % D < 6 ? 1 : 2;
    worst[kind] = std::fmax(worst[kind], std::fabs(v.scale[a] * (v.y[a] - (double)y[i])));
  }
  std::printf("executor against dense: step differs by %.3g rad, %.3g map units, %.3g log-scale (bounds %.3g %.3g %.3g)\n",
              worst[0], worst[1], worst[2], tol[0], tol[1], tol[2]);
  for (int k = 0; k < 3; ++k) CHECK(worst[k] <= tol[k], "executor against dense, kind %d: %.3g > %.3g", k, worst[k], tol[k]);
}

int main(int argc, char** argv) {
  RandomCalls();
  StatusRules();
  ArgumentErrors();
  if (argc > 1) ExecutorAgainstDense(argv[1]);
  if (g_fail) {
    std::printf("posegraph_plan_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("posegraph_plan_check OK\n");
  return 0;
}
