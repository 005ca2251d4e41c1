// posegraph_plan.cpp — see posegraph_plan.h.
#include "posegraph_plan.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <numeric>

#include "common.h"

namespace sg {

namespace {

int Find(std::vector<int>& p, int a) {
  while (p[a] != a) a = p[a] = p[p[a]];
  return a;
}

// The block of column j (local) whose row is i (local), a call-wide block index; -1 when L has no such block.
int BlockOf(const PgPlan& pl, int col0, int j, int i) {
  const int b0 = pl.colptr[col0 + j], b1 = pl.colptr[col0 + j + 1];
  const auto first = pl.blk_row.begin() + b0, last = pl.blk_row.begin() + b1;
  const auto it = std::lower_bound(first, last, i);
  return (it != last && *it == i) ? (int)(it - pl.blk_row.begin()) : -1;
}

// Stable counting sort of (key, item) pairs into CSR form: ptr gets one entry per key appended (the caller has
// pushed the leading offset), items the items by key, within a key in the order given.
void AppendCsr(const std::vector<std::pair<int, int>>& pairs, int nkeys, std::vector<int32_t>* ptr,
               std::vector<int32_t>* items) {
  std::vector<int> cnt((size_t)nkeys + 1, 0);
  for (const auto& p : pairs) cnt[p.first + 1] += 1;
  for (int k = 0; k < nkeys; ++k) cnt[k + 1] += cnt[k];
  const size_t base = items->size();
  items->resize(base + pairs.size());
  std::vector<int> at(cnt.begin(), cnt.end() - 1);
  for (const auto& p : pairs) (*items)[base + at[p.first]++] = p.second;
  for (int k = 0; k < nkeys; ++k) ptr->push_back((int32_t)(base + cnt[k + 1]));
}

}  // namespace

void PlanPoseGraph(const sg_map* mp, const int32_t* node_frame, const int32_t* node_fixed, const int32_t* node_offset,
                   const int32_t* edge_ab, const double* edge_meas, const double* edge_weight,
                   const int32_t* edge_offset, int32_t n, const sg_posegraph_options* o, PgPlan* out) {
  SG_REQUIRE(mp && o && out, SG_EINVAL, "null argument");
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative graph count");
  SG_REQUIRE(o->range >= 0.0 && std::isfinite(o->range), SG_EINVAL, "range must be 0 or positive");
  *out = PgPlan{};
  PgPlan& pl = *out;
  pl.fix_scale = o->fix_scale != 0;
  pl.D = pl.fix_scale ? 6 : 7;
  pl.b = o->range * o->range;
  pl.inv_b = pl.b > 0.0 ? 1.0 / pl.b : 0.0;
  pl.colptr.push_back(0);
  pl.asm_ptr.push_back(0);
  pl.gasm_ptr.push_back(0);
  pl.upd_ptr.push_back(0);
  if (n == 0) return;
  SG_REQUIRE(node_offset && edge_offset, SG_EINVAL, "null offsets");
  SG_REQUIRE(node_offset[0] == 0 && edge_offset[0] == 0, SG_EINVAL, "offsets must start at 0");
  for (int g = 0; g < n; ++g) {
    SG_REQUIRE(node_offset[g + 1] >= node_offset[g] && edge_offset[g + 1] >= edge_offset[g], SG_EINVAL,
               "decreasing offset");
    SG_REQUIRE(node_offset[g + 1] - node_offset[g] <= kPgMaxNodes, SG_EINVAL, "too many nodes in a graph");
    SG_REQUIRE(edge_offset[g + 1] - edge_offset[g] <= kPgMaxEdges, SG_EINVAL, "too many edges in a graph");
  }
  const int NT = node_offset[n], ET = edge_offset[n];
  SG_REQUIRE(NT <= kPgMaxCallNodes && ET <= kPgMaxCallEdges, SG_EINVAL, "too many nodes or edges in a call");
  SG_REQUIRE(NT == 0 || (node_frame && node_fixed), SG_EINVAL, "null node list");
  SG_REQUIRE(ET == 0 || (edge_ab && edge_meas && edge_weight), SG_EINVAL, "null edge list");
  const sg_map& m = *mp;
  SG_REQUIRE(m.num_frames >= 0 && m.num_points >= 0 && m.num_obs >= 0, SG_EINVAL, "negative map sizes");
  SG_REQUIRE(NT == 0 || (m.q && m.t), SG_EINVAL, "the map's poses cannot be read");
  if (o->move_points && m.num_obs > 0) {
    SG_REQUIRE(m.X && m.obs_frame && m.obs_point && m.obs_disabled, SG_EINVAL,
               "move_points: the map's points and observations cannot be read");
    for (int i = 0; i < m.num_obs; ++i)
      SG_REQUIRE(m.obs_frame[i] >= 0 && m.obs_frame[i] < m.num_frames && m.obs_point[i] >= 0 &&
                     m.obs_point[i] < m.num_points,
                 SG_EINVAL, "move_points: observation index out of range");
  }
  std::vector<uint8_t> seen((size_t)m.num_frames, 0);
  for (int i = 0; i < NT; ++i) {
    SG_REQUIRE(node_frame[i] >= 0 && node_frame[i] < m.num_frames, SG_EINVAL, "frame index out of range");
    SG_REQUIRE(!seen[node_frame[i]], SG_EINVAL, "frame listed twice");
    seen[node_frame[i]] = 1;
  }
  for (int g = 0; g < n; ++g) {
    const int nn = node_offset[g + 1] - node_offset[g];
    for (int e = edge_offset[g]; e < edge_offset[g + 1]; ++e) {
      const int a = edge_ab[2 * (size_t)e], b = edge_ab[2 * (size_t)e + 1];
      SG_REQUIRE(a >= 0 && a < nn && b >= 0 && b < nn, SG_EINVAL, "edge node index out of range");
      SG_REQUIRE(a != b, SG_EINVAL, "an edge of one node");
      const double* q = edge_meas + 8 * (size_t)e;
      const double n2 = (q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]);
      SG_REQUIRE(std::fabs(n2 - 1.0) <= 1e-9, SG_EINVAL, "an edge's q is not a unit quaternion");   // (false for NaN)
      SG_REQUIRE(std::isfinite(q[4]) && std::isfinite(q[5]) && std::isfinite(q[6]) && std::isfinite(q[7]), SG_EINVAL,
                 "an edge's u or rho is not finite");
      const double* w = edge_weight + 3 * (size_t)e;
      for (int k = 0; k < (pl.fix_scale ? 2 : 3); ++k)
        SG_REQUIRE(w[k] > 0.0 && std::isfinite(w[k]), SG_EINVAL, "an edge weight is not positive and finite");
    }
  }
  // the call's lists as the kernel reads them
  pl.graphs.assign((size_t)n, PgGraph{});
  pl.node_frame.assign(node_frame, node_frame + NT);
  pl.node_col.assign((size_t)NT, -1);
  pl.edge_ab.assign(edge_ab, edge_ab + 2 * (size_t)ET);
  pl.edge_meas.assign(edge_meas, edge_meas + 8 * (size_t)ET);
  pl.edge_w.assign(edge_weight, edge_weight + 3 * (size_t)ET);
  pl.x0.assign((size_t)kPgState * NT, 0.0);
  for (int i = 0; i < NT; ++i) {
    for (int k = 0; k < 4; ++k) pl.x0[kPgState * (size_t)i + k] = m.q[4 * (size_t)node_frame[i] + k];
    for (int k = 0; k < 3; ++k) pl.x0[kPgState * (size_t)i + 4 + k] = m.t[3 * (size_t)node_frame[i] + k];
  }
  for (int g = 0; g < n; ++g) {
    PgGraph& G = pl.graphs[g];
    G.node0 = node_offset[g];
    G.nn = node_offset[g + 1] - G.node0;
    G.edge0 = edge_offset[g];
    G.ne = edge_offset[g + 1] - G.edge0;
    G.col0 = (int32_t)pl.col_node.size();
    G.blk0 = (int32_t)pl.blk_row.size();
    const int32_t* fixed = node_fixed + G.node0;
    const int32_t* ab = edge_ab + 2 * (size_t)G.edge0;
    // status: DID_NOT_RUN before NO_ANCHOR
    int nfree = 0;
    for (int i = 0; i < G.nn; ++i) nfree += fixed[i] == 0;
    bool touched = false;
    for (int e = 0; e < G.ne; ++e) touched = touched || !fixed[ab[2 * e]] || !fixed[ab[2 * e + 1]];
    G.status = SG_PG_OK;
    if (nfree == 0 || !touched) {
      G.status = SG_PG_DID_NOT_RUN;
    } else {
      std::vector<int> par((size_t)G.nn);
      std::iota(par.begin(), par.end(), 0);
      for (int e = 0; e < G.ne; ++e) par[Find(par, ab[2 * e])] = Find(par, ab[2 * e + 1]);
      std::vector<uint8_t> has_free((size_t)G.nn, 0), has_fixed((size_t)G.nn, 0);
      for (int i = 0; i < G.nn; ++i) (fixed[i] ? has_fixed : has_free)[Find(par, i)] = 1;
      for (int i = 0; i < G.nn; ++i)
        if (has_free[i] && !has_fixed[i]) G.status = SG_PG_NO_ANCHOR;
    }
    G.run = G.status == SG_PG_OK;
    if (!G.run) continue;
    pl.num_run += 1;
    // elimination order: greedy minimum degree with an exact fill simulation
    std::vector<int> fr, fi_of((size_t)G.nn, -1);
    for (int i = 0; i < G.nn; ++i)
      if (!fixed[i]) {
        fi_of[i] = (int)fr.size();
        fr.push_back(i);
      }
    const int nf = (int)fr.size();
    std::vector<uint8_t> adj((size_t)nf * nf, 0), gone((size_t)nf, 0);
    std::vector<int> deg((size_t)nf, 0);
    for (int e = 0; e < G.ne; ++e) {
      const int a = fi_of[ab[2 * e]], b = fi_of[ab[2 * e + 1]];
      if (a < 0 || b < 0 || adj[(size_t)a * nf + b]) continue;
      adj[(size_t)a * nf + b] = adj[(size_t)b * nf + a] = 1;
      deg[a] += 1;
      deg[b] += 1;
    }
    std::vector<std::vector<int>> below((size_t)nf);   // per column, the free-node indices of its rows
    std::vector<int> col_of((size_t)nf, -1);
    for (int j = 0; j < nf; ++j) {
      int v = -1;
      for (int i = 0; i < nf; ++i)
        if (!gone[i] && (v < 0 || deg[i] < deg[v])) v = i;
      col_of[v] = j;
      gone[v] = 1;
      std::vector<int>& nb = below[j];
      for (int i = 0; i < nf; ++i)
        if (!gone[i] && adj[(size_t)v * nf + i]) nb.push_back(i);
      for (size_t p = 0; p < nb.size(); ++p) {
        deg[nb[p]] -= 1;
        for (size_t q = p + 1; q < nb.size(); ++q)
          if (!adj[(size_t)nb[p] * nf + nb[q]]) {
            adj[(size_t)nb[p] * nf + nb[q]] = adj[(size_t)nb[q] * nf + nb[p]] = 1;
            deg[nb[p]] += 1;
            deg[nb[q]] += 1;
          }
      }
      pl.col_node.push_back(fr[v]);
      pl.node_col[G.node0 + fr[v]] = j;
    }
    G.nc = nf;
    // symbolic factorisation: the diagonal, then the rows ascending
    for (int j = 0; j < nf; ++j) {
      std::vector<int> rows;
      for (int i : below[j]) rows.push_back(col_of[i]);
      std::sort(rows.begin(), rows.end());
      pl.blk_row.push_back(j);
      pl.blk_col.push_back(j);
      for (int r : rows) {
        pl.blk_row.push_back(r);
        pl.blk_col.push_back(j);
      }
      pl.colptr.push_back((int32_t)pl.blk_row.size());
      SG_REQUIRE(pl.blk_row.size() <= (size_t)kPgMaxCallBlocks, SG_EINVAL, "too many blocks in the call's factors");
    }
    G.nb = (int32_t)pl.blk_row.size() - G.blk0;
    // assembly lists in listed edge order
    std::vector<std::pair<int, int>> hb, gb;
    for (int e = 0; e < G.ne; ++e) {
      const int ca = pl.node_col[G.node0 + ab[2 * e]], cb = pl.node_col[G.node0 + ab[2 * e + 1]];
      if (ca >= 0) {
        hb.emplace_back(pl.colptr[G.col0 + ca] - G.blk0, 4 * e + 0);
        gb.emplace_back(ca, 2 * e + 0);
      }
      if (cb >= 0) {
        hb.emplace_back(pl.colptr[G.col0 + cb] - G.blk0, 4 * e + 1);
        gb.emplace_back(cb, 2 * e + 1);
      }
      if (ca >= 0 && cb >= 0) {
        const int B = ca > cb ? BlockOf(pl, G.col0, cb, ca) : BlockOf(pl, G.col0, ca, cb);
        SG_REQUIRE(B >= 0, SG_EINVAL, "internal: an edge's block is missing from the pattern");
        hb.emplace_back(B - G.blk0, 4 * e + (ca > cb ? 2 : 3));
      }
    }
    AppendCsr(hb, G.nb, &pl.asm_ptr, &pl.asm_items);
    AppendCsr(gb, G.nc, &pl.gasm_ptr, &pl.gasm_items);
    // update lists
    for (int j = 0; j < nf; ++j) {
      const int b0 = pl.colptr[G.col0 + j], b1 = pl.colptr[G.col0 + j + 1];
      for (int p = b0 + 1; p < b1; ++p)
        for (int q = p; q < b1; ++q) {
          const int T = BlockOf(pl, G.col0, pl.blk_row[p], pl.blk_row[q]);
          SG_REQUIRE(T >= 0, SG_EINVAL, "internal: an update's target is missing from the pattern");
          pl.upd.push_back(q);
          pl.upd.push_back(p);
          pl.upd.push_back(T);
        }
      SG_REQUIRE(pl.upd.size() / 3 <= (size_t)kPgMaxCallUpdates, SG_EINVAL, "too many factor updates in the call");
      pl.upd_ptr.push_back((int32_t)(pl.upd.size() / 3));
    }
  }
}

size_t PgPlan::WorkspaceDoubles() const {
  const size_t B = blk_row.size(), E = edge_ab.size() / 2, N = node_col.size(), C = col_node.size();
  return kPgBlk * B + 2 * (size_t)kPgRec * E + 2 * (size_t)kPgState * N + 6 * 7 * C + 8;
}

PgView PgPlan::View(double* ws) const {
  const size_t B = blk_row.size(), E = edge_ab.size() / 2, N = node_col.size(), C = col_node.size();
  PgView v{};
  v.graphs = graphs.data();
  v.node_col = node_col.data();
  v.col_node = col_node.data();
  v.edge_ab = edge_ab.data();
  v.edge_meas = edge_meas.data();
  v.edge_w = edge_w.data();
  v.colptr = colptr.data();
  v.blk_row = blk_row.data();
  v.blk_col = blk_col.data();
  v.asm_ptr = asm_ptr.data();
  v.asm_items = asm_items.data();
  v.gasm_ptr = gasm_ptr.data();
  v.gasm_items = gasm_items.data();
  v.upd_ptr = upd_ptr.data();
  v.upd = upd.data();
  double* p = ws;
  v.L = p; p += kPgBlk * B;
  v.rec[0] = p; p += (size_t)kPgRec * E;
  v.rec[1] = p; p += (size_t)kPgRec * E;
  v.x[0] = p; p += (size_t)kPgState * N;
  v.x[1] = p; p += (size_t)kPgState * N;
  v.g = p; p += 7 * C;
  v.hd = p; p += 7 * C;
  v.scale = p; p += 7 * C;
  v.diag = p; p += 7 * C;
  v.y = p; p += 7 * C;
  v.delta = p;
  v.D = D;
  v.fix_scale = fix_scale;
  v.b = b;
  v.inv_b = inv_b;
  std::copy(x0.begin(), x0.end(), v.x[0]);
  return v;
}

bool PgCpuFactorSolve(const PgView& v, const PgGraph& G) {
  const int D = v.D, dd = D * D;
  for (int j = 0; j < G.nc; ++j) {
    if (!PgFactorDiag(v, G, j)) return false;
    const int rows = v.colptr[G.col0 + j + 1] - v.colptr[G.col0 + j] - 1;
    for (int i = 0; i < rows * D; ++i) PgSolveOffRow(v, G, j, i);
    const int nu = v.upd_ptr[G.col0 + j + 1] - v.upd_ptr[G.col0 + j];
    for (int i = 0; i < nu * dd; ++i) PgUpdateEntry(v, G, j, i);
  }
  for (int j = 0; j < G.nc; ++j) {
    PgForwardDiag(v, G, j);
    const int rows = v.colptr[G.col0 + j + 1] - v.colptr[G.col0 + j] - 1;
    for (int i = 0; i < rows * D; ++i) PgForwardRow(v, G, j, i);
  }
  for (int j = G.nc - 1; j >= 0; --j) {
    for (int c = 0; c < D; ++c) PgBackwardGather(v, G, j, c);
    PgBackwardDiag(v, G, j);
  }
  return true;
}

namespace {
// One sweep over the graph's edges at x[slot]: the linearization into rec[slot], the cost and the fixed cost.
void Sweep(const PgView& v, const PgGraph& G, int slot, double* cost, double* fixed_cost) {
  *cost = *fixed_cost = 0.0;
  for (int e = 0; e < G.ne; ++e) {
    bool fx;
    const double c = PgEdgeLinearize(v, G, e, slot, &fx);
    *(fx ? fixed_cost : cost) += c;
  }
}
}  // namespace

// Ceres 1.8's TrustRegionMinimizer and LevenbergMarquardtStrategy as ba_lm.h restates them for the device
// (fin_push, fin_count, decide_step), on the host.
void PgCpuSolve(const PgView& v, const PgGraph& G, const sg_solver_options& o, PgOut* out) {
  const int D = v.D, nx = G.nc * D, dd = D * D;
  const bool dis = o.disable_termination != 0;
  int cur = 0, need_lin = 1, first = 1, done = 0, ok = 1, term = SG_NO_CONVERGENCE;
  int pushed = 0, lm_iters = 0, n_succ = 0, n_unsucc = 0, n_invalid = 0, consecutive_invalid = 0, reuse_diag = 0;
  double radius = o.initial_trust_region_radius, decrease_factor = 2.0;
  double cost = 0.0, fixed_cost = 0.0, initial_cost = 0.0, x_norm = 0.0, abs_gtol = 0.0, min_pushed = 0.0;
  double slot_cost[2] = {0.0, 0.0}, fx0 = 0.0;
  Sweep(v, G, 0, &slot_cost[0], &fx0);
  const long long cap =
      (long long)std::max(o.max_num_iterations, 0) * (std::max(o.max_num_consecutive_invalid_steps, 0) + 2) + 16;
  for (long long it = 0; it < cap && !done; ++it) {
    if (need_lin) {
      double gmax = 0.0;
      for (int i = 0; i < nx; ++i) {
        PgGradEntry(v, G, i, cur);
        gmax = std::fmax(gmax, std::fabs(v.g[7 * (size_t)(G.col0 + i / D) + i % D]));
      }
      if (first) {
        for (int i = 0; i < nx; ++i) {
          const size_t a = 7 * (size_t)(G.col0 + i / D) + i % D;
          v.scale[a] = o.jacobi_scaling ? 1.0 / (1.0 + std::sqrt(v.hd[a])) : 1.0;
        }
        fixed_cost = fx0;
        cost = slot_cost[cur];
        initial_cost = cost + fixed_cost;
        abs_gtol = o.gradient_tolerance * gmax;
        pushed = 1;
        min_pushed = cost;
        double xn = 0.0;
        for (int nd = 0; nd < G.nn; ++nd) xn += PgNodeNorm2(v, G, nd, cur);
        x_norm = std::sqrt(xn);
        if (gmax <= abs_gtol && !dis) { done = 1; ok = 1; term = SG_GRADIENT_TOLERANCE; }
        first = 0;
      } else {
        cost = slot_cost[cur];
        if (!dis && gmax <= abs_gtol) { done = 1; ok = 1; term = SG_GRADIENT_TOLERANCE; }
        else if (!dis && radius < o.min_trust_region_radius) { done = 1; ok = 1; term = SG_PARAMETER_TOLERANCE; }
        else { pushed += 1; min_pushed = std::fmin(min_pushed, cost); }
      }
      need_lin = 0;
    }
    if (!done) {
      if (!dis && pushed - 1 >= o.max_num_iterations) { done = 1; ok = 1; term = SG_NO_CONVERGENCE; }
      else if (dis && lm_iters >= o.max_num_iterations) { done = 1; ok = 1; term = SG_NO_CONVERGENCE; }
    }
    if (done) break;
    lm_iters += 1;
    for (int i = 0; i < nx; ++i) {
      const size_t a = 7 * (size_t)(G.col0 + i / D) + i % D;
      if (!reuse_diag)
        v.diag[a] = std::fmin(std::fmax(v.scale[a] * v.scale[a] * v.hd[a], o.min_lm_diagonal), o.max_lm_diagonal);
      v.y[a] = v.g[a] * v.scale[a];
    }
    for (int i = 0; i < G.nb * dd; ++i) PgAssembleEntry(v, G, i, cur, radius);
    const bool solved_lin = PgCpuFactorSolve(v, G);
    double model = 0.0, sums[2] = {0.0, 0.0}, cand_cost = 0.0, fxc = 0.0;
    if (solved_lin) {
      for (int nd = 0; nd < G.nn; ++nd) PgCandidateNode(v, G, nd, cur, sums);
      for (int e = 0; e < G.ne; ++e) model += PgModelEdge(v, G, e, cur);
      Sweep(v, G, cur ^ 1, &cand_cost, &fxc);
      slot_cost[cur ^ 1] = cand_cost;
    }
    // decide_step
    const bool solved = solved_lin && std::isfinite(sums[0]) && std::isfinite(model);
    const bool valid = solved && !(model < 0.0);
    bool rejected = true;
    if (!valid) {
      n_invalid += 1;
      consecutive_invalid += 1;
      if (!dis && consecutive_invalid >= o.max_num_consecutive_invalid_steps) {
        done = 1; ok = 0; term = SG_NUMERICAL_FAILURE;
        break;
      }
    } else {
      consecutive_invalid = 0;
      const double new_cost = cand_cost, step_norm = std::sqrt(sums[0]);
      if (!dis && step_norm <= o.parameter_tolerance * (x_norm + o.parameter_tolerance)) {
        done = 1; ok = 1; term = SG_PARAMETER_TOLERANCE;
        break;
      }
      const double cost_change = cost - new_cost;
      if (!dis && std::fabs(cost_change) < o.function_tolerance * cost) {
        done = 1; ok = 1; term = SG_FUNCTION_TOLERANCE;
        break;
      }
      const double rel = cost_change / model;
      if (rel > o.min_relative_decrease) {
        n_succ += 1;
        const double t = 2.0 * rel - 1.0;
        radius = std::fmin(o.max_trust_region_radius, radius / std::fmax(1.0 / 3.0, 1.0 - t * t * t));
        decrease_factor = 2.0;
        reuse_diag = 0;
        cur ^= 1;
        x_norm = std::sqrt(sums[1]);
        cost = new_cost;
        need_lin = 1;
        rejected = false;
      }
    }
    if (rejected) {
      n_unsucc += 1;
      radius = radius / decrease_factor;
      decrease_factor *= 2.0;
      reuse_diag = 1;
      if (!dis && radius < o.min_trust_region_radius) {
        done = 1; ok = 1; term = SG_PARAMETER_TOLERANCE;
        break;
      }
      if (o.always_linearize) {
        need_lin = 1;
      } else {
        pushed += 1;
        min_pushed = std::fmin(min_pushed, cost);
      }
    }
  }
  out->initial_cost = initial_cost;
  out->final_cost = min_pushed + fixed_cost;
  out->fixed_cost = fixed_cost;
  out->radius = radius;
  out->num_iterations = pushed;
  out->n_succ = n_succ;
  out->n_unsucc = n_unsucc;
  out->n_invalid = n_invalid;
  out->termination = term;
  out->ok = ok;
  out->lm_iters = lm_iters;
  out->finished = done;
  out->cur = cur;
  out->pad = 0;
}

void PgWriteBack(sg_map* m, const PgPlan& plan, const int32_t* status, const double* xres, int move_points,
                 double* log_scale) {
  const int n = (int)plan.graphs.size();
  // unit quaternions with w >= 0 of the solved nodes
  std::vector<double> qn(4 * plan.node_col.size(), 0.0);
  for (int g = 0; g < n; ++g) {
    const PgGraph& G = plan.graphs[g];
    for (int i = G.node0; i < G.node0 + G.nn; ++i) {
      if (log_scale) log_scale[i] = 0.0;
      if (status[g] != SG_PG_OK || plan.node_col[i] < 0) continue;
      const double* x = xres + kPgState * (size_t)i;
      double rn = 1.0 / std::sqrt((x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]));
      if (x[3] < 0.0) rn = -rn;
      for (int k = 0; k < 4; ++k) qn[4 * (size_t)i + k] = x[k] * rn;
      if (log_scale) log_scale[i] = x[7];
    }
  }
  if (move_points && m->num_obs > 0) {
    // every point moves with its anchor: the node frame of its first enabled observation in a node of an OK graph
    std::vector<int32_t> frame_node((size_t)m->num_frames, -1), anchor((size_t)m->num_points, -1);
    for (int g = 0; g < n; ++g)
      if (status[g] == SG_PG_OK)
        for (int i = plan.graphs[g].node0; i < plan.graphs[g].node0 + plan.graphs[g].nn; ++i)
          frame_node[plan.node_frame[i]] = i;
    for (int i = 0; i < m->num_obs; ++i) {
      if (m->obs_disabled[i] || frame_node[m->obs_frame[i]] < 0 || anchor[m->obs_point[i]] >= 0) continue;
      anchor[m->obs_point[i]] = frame_node[m->obs_frame[i]];
    }
    for (int p = 0; p < m->num_points; ++p) {
      const int i = anchor[p];
      if (i < 0 || plan.node_col[i] < 0) continue;   // a fixed anchor does not move
      const double* xo = plan.x0.data() + kPgState * (size_t)i;
      const double* xn = xres + kPgState * (size_t)i;
      double* X = m->X + 4 * (size_t)p;
      // xyz <- lambda R_new^T R_old (xyz - W t_old) + W t_new
      const double d[3] = {X[0] - X[3] * xo[4], X[1] - X[3] * xo[5], X[2] - X[3] * xo[6]};
      const double cq[4] = {-qn[4 * (size_t)i], -qn[4 * (size_t)i + 1], -qn[4 * (size_t)i + 2], qn[4 * (size_t)i + 3]};
      double pc[3], pw[3];
      PgRotate(xo, d, pc);
      PgRotate(cq, pc, pw);
      const double lam = std::exp(xn[7]);
      for (int k = 0; k < 3; ++k) X[k] = lam * pw[k] + X[3] * xn[4 + k];
    }
  }
  for (int g = 0; g < n; ++g) {
    const PgGraph& G = plan.graphs[g];
    if (status[g] != SG_PG_OK) continue;
    for (int i = G.node0; i < G.node0 + G.nn; ++i) {
      if (plan.node_col[i] < 0) continue;
      const int f = plan.node_frame[i];
      for (int k = 0; k < 4; ++k) m->q[4 * (size_t)f + k] = qn[4 * (size_t)i + k];
      for (int k = 0; k < 3; ++k) m->t[3 * (size_t)f + k] = xres[kPgState * (size_t)i + 4 + k];
    }
  }
}

}  // namespace sg
