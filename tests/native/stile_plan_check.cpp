// stile_plan_check.cpp — CPU check of PlanStile (slam-robot_amd/csrc/ba_plan.cpp): where k_S_reduce's band tiles go in
// St, the tile-major copy of S that k_chol_tiles loads, and the reversed band ends of its bottom workgroup.  On
// generated sliding-window problems (as tests/native/ba_plan_check.cpp), with and without padding of the last tile,
// split and not: the slots are in range, no two tiles share one, they cover exactly the tiles each workgroup
// reads, every element a workgroup loads from St is the one its loader takes from row-major S (both modelled
// here with symbolic values), and the planned band ends are what the kernel's own search derives.  Built
// stand-alone with -fsanitize=address,undefined by tests/test_stile_plan.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "ba_plan.h"
#include "common.h"

using namespace sg;

static int g_fail = 0;
static std::string g_case;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      if (++g_fail <= 40) printf("FAIL [%s] %s:%d: %s\n", g_case.c_str(), __FILE__, __LINE__, #cond); \
    }                                                                                    \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(s >> 33);
  }
  int range(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }   // inclusive
};

// frames in a row, the first nfixed constant, FrameDistance between neighbours, each point seen in a run of rmin ..
// rmax consecutive frames
struct Prob {
  int F = 0;
  std::vector<uint8_t> rot_free, trans_free, point_free;
  std::vector<int32_t> frame_camera, frame_index, point_index, obs_frame, obs_point, dist_frame, dist_prev;
  std::vector<double> k, q, t, X, obs_pt;
  sg_problem view() {
    sg_problem p{};
    p.num_cameras = 1;
    p.k = k.data();
    p.num_frames = F;
    p.q = q.data();
    p.t = t.data();
    p.frame_camera = frame_camera.data();
    p.frame_rot_free = rot_free.data();
    p.frame_trans_free = trans_free.data();
    p.frame_map_index = frame_index.data();
    p.num_points = (int)point_free.size();
    p.X = X.data();
    p.point_free = point_free.data();
    p.point_map_index = point_index.data();
    p.num_obs = (int)obs_frame.size();
    p.obs_pt = obs_pt.data();
    p.obs_frame = obs_frame.data();
    p.obs_point = obs_point.data();
    p.num_dist = (int)dist_frame.size();
    p.dist_frame = dist_frame.data();
    p.dist_prev = dist_prev.data();
    p.range = 2.0;
    p.dist_target = 150.0;
    p.dist_range = 15.0;
    p.stab_range = 5.0;
    return p;
  }
};
static Prob MakeProb(Rng* r, int F, int nfixed, int points, int rmin, int rmax) {
  Prob pr;
  pr.F = F;
  pr.rot_free.assign(F, 1);
  pr.trans_free.assign(F, 1);
  for (int f = 0; f < nfixed; ++f) pr.rot_free[f] = pr.trans_free[f] = 0;
  pr.frame_camera.assign(F, 0);
  pr.frame_index.assign(F, -1);
  pr.k.assign(7, 1.0);
  pr.q.assign(4 * (size_t)F, 0.0);
  pr.t.assign(3 * (size_t)F, 0.0);
  for (int f = 1; f < F; ++f) {
    pr.dist_frame.push_back(f);
    pr.dist_prev.push_back(f - 1);
  }
  for (int i = 0; i < points; ++i) {
    const int len = std::min(r->range(rmin, rmax), F);
    const int f0 = r->range(0, F - len);
    for (int f = f0; f < f0 + len; ++f) {
      pr.obs_frame.push_back(f);
      pr.obs_point.push_back(i);
      pr.obs_pt.push_back(0.0);
      pr.obs_pt.push_back(0.0);
    }
    pr.point_free.push_back(1);
  }
  pr.point_index.assign(points, -1);
  pr.X.assign(4 * (size_t)points, 1.0);
  return pr;
}

struct Plan {
  Order o;
  WorkLists w;
  Envelope e;
};
static Plan MakePlan(const sg_problem& p) {
  Plan pl;
  PlanBlocks(p, &pl.o);
  PlanPointOrder(p, &pl.o);
  PlanObservations(p, &pl.o);
  PlanSweep(pl.o, 256, 0, &pl.w);
  PlanSchur(pl.o, 256, &pl.w);
  PlanReduceLists(pl.o, &pl.w);
  PlanFrameDistance(p, pl.o, &pl.w);
  PlanIntrLists(pl.o, &pl.w);
  PlanLoBlk(pl.o, &pl.w);
  pl.e = PlanEnvelope(pl.o, pl.w.lo_blk, pl.w.segs, pl.w.nseg);
  return pl;
}

// symbolic values: 0 and 1 the constants, element (i, j) of S as 2 + i n + j
static int64_t Sym(int i, int j, int n) { return 2 + (int64_t)i * n + j; }

static void CheckStile(const char* name, const Plan& pl, const CholPlan& c) {
  g_case = name;
  const Envelope& e = pl.e;
  const int n = pl.o.n, NT = e.npanel;
  const StilePlan sp = PlanStile(e, c);
  printf("[%s] n %d NT %d (padding %d) stiles %d: nd %d ns %d\n", name, n, NT, 16 * NT - n, e.nstile, c.nd, c.ns);
  CHECK(c.tiles && !c.border);
  CHECK((int)sp.dst.size() == 2 * std::max(e.nstile, 1) && (int)sp.tend_rev.size() == NT);
  const int ns = c.ns, nd = c.nd, m = nd > 0 ? NT - nd - ns : NT, top_end = nd > 0 ? m + ns : NT;
  std::vector<int> tend(NT);
  for (int R = 0; R < NT; ++R) tend[R] = std::min(NT, (e.panel_jmax[R] + kCholNb - 1) / kCholNb);
  auto in_band = [&](int R, int C) { return R >= 0 && R <= C && C < NT && C < tend[R]; };

  // in range, one slot per tile, no slot twice, never the zero slot
  std::set<int> used;
  std::set<std::pair<int, int>> band;
  for (int t = 0; t < e.nstile; ++t) {
    const int R = e.stile[t] >> 16, C = e.stile[t] & 0xffff;
    band.insert({R, C});
    CHECK(in_band(R, C));
    const int top = sp.dst[2 * t], bot = sp.dst[2 * t + 1];
    CHECK((top >= 0) != (bot >= 0));
    CHECK(top == -1 || (top >= 0 && top < NT * kTB));
    CHECK(bot == -1 || (bot >= NT * kTB && bot < 2 * NT * kTB));
    for (int s : {top, bot})
      if (s >= 0) CHECK(used.insert(s).second);
    // exactly the tiles each workgroup reads: the top rows and columns < m + ns, the bottom columns >= m + ns
    CHECK((top >= 0) == (R < top_end && C < top_end));
    CHECK((bot >= 0) == (C >= top_end));
    if (top >= 0) CHECK(top == R * kTB + (C - R));
    if (bot >= 0) CHECK(bot == NT * kTB + (NT - 1 - C) * kTB + (C - R) && R >= m);
  }
  for (int R = 0; R < NT; ++R)
    for (int C = R; C < NT; ++C) CHECK(in_band(R, C) == (band.count({R, C}) == 1));
  CHECK((size_t)2 * NT * kTB * 256 + 256 == stile_doubles(NT));

  // St as k_S_reduce's tile workgroups fill it (thread (ti, tj) of tile (R, C): its element of S, 0 below the
  // diagonal, the identity past n), symbolically
  std::vector<int64_t> St(stile_doubles(NT), 0);
  for (int t = 0; t < e.nstile; ++t) {
    const int R = e.stile[t] >> 16, C = e.stile[t] & 0xffff;
    for (int ti = 0; ti < 16; ++ti)
      for (int tj = 0; tj < 16; ++tj) {
        const int i = 16 * R + ti, j = 16 * C + tj;
        const bool live = i < n && j < n;
        const int64_t v = live ? (i <= j ? Sym(i, j, n) : 0) : (i == j ? 1 : 0);
        if (sp.dst[2 * t] >= 0) St[(size_t)256 * sp.dst[2 * t] + stile_elem(ti, tj)] = v;
        if (sp.dst[2 * t + 1] >= 0) St[(size_t)256 * sp.dst[2 * t + 1] + stile_elem(15 - tj, 15 - ti)] = v;
      }
  }
  // row-major S as k_S_reduce leaves it, and the loader of it (k_chol_tiles' tile_load without St)
  auto S_at = [&](int si, int sj) -> int64_t { return in_band(si >> 4, sj >> 4) && si <= sj ? Sym(si, sj, n) : 0; };
  auto old_load = [&](bool rev, int sep, int I, int J, int a, int b) -> int64_t {
    const int np = 16 * NT, gi = 16 * I + a, gj = 16 * J + b;
    const bool zsep = I >= sep && J >= sep;
    const int si = rev ? np - 1 - gj : gi, sj = rev ? np - 1 - gi : gj;
    const bool in = I >= 0 && si < n && sj < n && !zsep;
    return in ? S_at(si, sj) : ((gi == gj && !zsep) ? 1 : 0);
  };
  auto new_load = [&](int sbase, int srow, int scol, int I, int J, int a, int b) -> int64_t {
    const bool in = I >= 0 && I < srow && J < scol;
    const size_t slot = in ? sbase + I * kTB + (J - I) : 2 * NT * kTB;
    CHECK(slot * 256 + 255 < St.size());
    return St[slot * 256 + stile_elem(a, b)];
  };
  // every tile a wave can hold for a column it works on (rows J - 7 .. J), both workgroups
  for (int wg = 0; wg < (nd > 0 ? 2 : 1); ++wg) {
    const bool rev = wg == 1;
    const int NTf = rev ? nd + ns : top_end;
    for (int J = 0; J < NTf; ++J)
      for (int I = J - (kTB - 1); I <= J; ++I)
        for (int a = 0; a < 16; ++a)
          for (int b = 0; b < 16; ++b) {
            CHECK(old_load(rev, rev ? nd : 1 << 28, I, J, a, b) ==
                  new_load(rev ? NT * kTB : 0, rev ? nd : NTf, NTf, I, J, a, b));
          }
  }
  // the reversed band ends: the kernel's search over the kTB rows above column c
  for (int k = 0; k < NT; ++k) {
    const int col = NT - 1 - k;
    int lo = col;
    for (int h = kTB - 1; h >= 0; --h) {
      const int i = col - kTB + h;
      if (i >= 0 && ((e.panel_jmax[std::max(0, i)] + 15) >> 4) > col) lo = i;
    }
    CHECK(sp.tend_rev[k] == NT - lo);
    CHECK(sp.tend_rev[k] > k && sp.tend_rev[k] <= k + kTB);
  }
}

int main() {
  Rng rng{20261019};
  const CholGrants grants{128 * 1024, 128 * 1024, 128 * 1024};
  struct Case {
    const char* name;
    int F, nfixed, points, rmin, rmax;
    bool split;
  };
  const Case cases[] = {
      {"n=204 NT=13 padded", 36, 2, 700, 2, 12, true},   {"n=240 NT=15", 44, 4, 800, 2, 8, true},
      {"n=102 NT=7 padded", 20, 3, 400, 2, 8, false},    {"n=528 NT=33", 90, 2, 1500, 2, 12, true},
      {"n=534 NT=34 padded", 91, 2, 1500, 2, 14, true},  {"n=96 NT=6", 18, 2, 300, 2, 10, false},
  };
  for (const Case& cs : cases) {
    Prob pr = MakeProb(&rng, cs.F, cs.nfixed, cs.points, cs.rmin, cs.rmax);
    const Plan pl = MakePlan(pr.view());
    const CholPlan c = PlanChol(pl.o, pl.e, grants, LoadKnobs());
    CheckStile(cs.name, pl, c);
    CHECK((c.nd > 0) == cs.split);
    if (cs.split) {
      LoadKnobs k7;
      k7.chol_sep7 = true;
      const CholPlan c7 = PlanChol(pl.o, pl.e, grants, k7);
      CHECK(c7.nd > 0 && c7.ns == kTB - 1);
      CheckStile((std::string(cs.name) + ", 7-row separator").c_str(), pl, c7);
      LoadKnobs k0;
      k0.chol_split = false;
      const CholPlan c0 = PlanChol(pl.o, pl.e, grants, k0);
      CHECK(c0.nd == 0);
      CheckStile((std::string(cs.name) + ", one workgroup").c_str(), pl, c0);
    }
  }
  if (g_fail) {
    printf("%d checks failed\n", g_fail);
    return 1;
  }
  printf("stile_plan_check OK\n");
  return 0;
}
