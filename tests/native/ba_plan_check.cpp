// ba_plan_check.cpp — CPU check of the load planner (slam-robot_amd/csrc/ba_plan.cpp): what the kernels' comments
// promise about the work lists, recomputed by brute force from generated sliding-window problems (frames in a
// row, the leading ones fixed, each point seen in a run of consecutive frames, FrameDistance pairs between
// consecutive frames, fixed seed).  Built stand-alone with -fsanitize=address,undefined by tests/test_ba_plan.py.
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <map>
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

// ---- problems
struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (uint32_t)(s >> 33);
  }
  int range(int lo, int hi) { return lo + (int)(next() % (uint32_t)(hi - lo + 1)); }   // inclusive
};

struct Prob {
  int F = 0, ncam = 1, cameras_free = 0;
  std::vector<uint8_t> rot_free, trans_free, point_free;
  std::vector<int32_t> frame_camera, frame_index, point_index, obs_frame, obs_point, dist_frame, dist_prev;
  std::vector<double> k, q, t, X, obs_pt;
  std::vector<std::pair<int, int>> runs;   // per point: first frame, frames
  sg_problem view() {
    sg_problem p{};
    p.num_cameras = ncam;
    p.k = k.data();
    p.cameras_free = cameras_free;
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

static Prob MakeFrames(int F, int nfixed, bool dist) {
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
  if (dist)
    for (int f = 1; f < F; ++f) {
      pr.dist_frame.push_back(f);
      pr.dist_prev.push_back(f - 1);
    }
  return pr;
}
static void AddPoint(Prob* pr, int f0, int len, bool free_pt) {
  pr->runs.emplace_back(f0, len);
  pr->point_free.push_back(free_pt);
}
static void AddRandomPoints(Prob* pr, Rng* r, int count, int rmin, int rmax, int flo, int fhi) {   // frames [flo, fhi)
  for (int i = 0; i < count; ++i) {
    const int len = std::min(r->range(rmin, rmax), fhi - flo);
    AddPoint(pr, r->range(flo, fhi - len), len, true);
  }
}
// observations in a shuffled order (the planner's orders must not rely on the problem's), values that name them
static void Finish(Prob* pr, Rng* r) {
  const int P = (int)pr->runs.size();
  std::vector<std::pair<int, int>> obs;
  for (int i = 0; i < P; ++i)
    for (int f = pr->runs[i].first; f < pr->runs[i].first + pr->runs[i].second; ++f) obs.emplace_back(f, i);
  for (size_t i = obs.size(); i > 1; --i) std::swap(obs[i - 1], obs[r->next() % i]);
  for (size_t o = 0; o < obs.size(); ++o) {
    pr->obs_frame.push_back(obs[o].first);
    pr->obs_point.push_back(obs[o].second);
    pr->obs_pt.push_back((double)o);
    pr->obs_pt.push_back(-(double)o);
  }
  pr->point_index.assign(P, -1);
  pr->X.resize(4 * (size_t)P);
  for (int i = 0; i < 4 * P; ++i) pr->X[i] = i;
}

// ---- the plan of one problem
struct Plan {
  Order o;
  WorkLists w;
  Envelope e;
};
static Plan MakePlan(const sg_problem& p, int ncu, const LoadKnobs& k) {
  Plan pl;
  PlanBlocks(p, &pl.o);
  PlanPointOrder(p, &pl.o);
  PlanObservations(p, &pl.o);
  PlanSweep(pl.o, ncu, k.lin_waves, &pl.w);
  PlanSchur(pl.o, ncu, &pl.w);
  PlanReduceLists(pl.o, &pl.w);
  PlanFrameDistance(p, pl.o, &pl.w);
  PlanIntrLists(pl.o, &pl.w);
  PlanLoBlk(pl.o, &pl.w);
  pl.e = PlanEnvelope(pl.o, pl.w.lo_blk, pl.w.segs, pl.w.nseg);
  return pl;
}

// What the checks below know of the problem, by brute force and in the problem's own numbering.
struct Truth {
  int NB = 0;
  std::vector<int> fb;                 // block of a frame, -1: constant
  std::vector<std::vector<int>> pobs;  // observations of a point, problem order
  std::vector<int> first, last;        // first / last free block of a point (NB / -1: none)
};
static Truth MakeTruth(const sg_problem& p) {
  Truth t;
  t.fb.assign(p.num_frames, -1);
  for (int f = 0; f < p.num_frames; ++f)
    if (p.frame_rot_free[f] || p.frame_trans_free[f]) t.fb[f] = t.NB++;
  t.pobs.resize(p.num_points);
  for (int o = 0; o < p.num_obs; ++o) t.pobs[p.obs_point[o]].push_back(o);
  t.first.assign(p.num_points, t.NB);
  t.last.assign(p.num_points, -1);
  for (int i = 0; i < p.num_points; ++i)
    for (int o : t.pobs[i]) {
      const int b = t.fb[p.obs_frame[o]];
      if (b < 0) continue;
      t.first[i] = std::min(t.first[i], b);
      t.last[i] = std::max(t.last[i], b);
    }
  return t;
}

static void CheckOrder(const sg_problem& p, const Truth& t, const Order& o) {
  const int P = p.num_points, M = p.num_obs;
  CHECK(o.NB == t.NB && o.nk == (p.cameras_free ? 7 * p.num_cameras : 0) && o.n == 6 * t.NB + o.nk);
  CHECK((int)o.point_perm.size() == P && (int)o.poff.size() == P + 1 && (int)o.obs_perm.size() == M);
  std::vector<int> seen(P, 0);
  for (int i = 0; i < P; ++i) {
    const int pt = o.point_perm[i];
    CHECK(pt >= 0 && pt < P && !seen[pt]++);
    CHECK(o.dfirst[i] == t.first[pt] && o.dlast[i] == t.last[pt]);
    if (i > 0) {   // sorted by first free block (no free block: the key NB, last), stable
      const int pp = o.point_perm[i - 1];
      CHECK(t.first[pp] < t.first[pt] || (t.first[pp] == t.first[pt] && pp < pt));
    }
    CHECK(o.pfree[i] == p.point_free[pt]);
    for (int a = 0; a < 4; ++a) CHECK(o.X[4 * i + a] == p.X[4 * pt + a]);
    CHECK(o.poff[i + 1] - o.poff[i] == (int)t.pobs[pt].size());
  }
  CHECK(o.poff[0] == 0 && o.poff[P] == M);
  std::vector<int> oseen(M, 0);
  for (int i = 0; i < P; ++i)
    for (int d = o.poff[i]; d < o.poff[i + 1]; ++d) {
      const int src = o.obs_perm[d];
      CHECK(src >= 0 && src < M && !oseen[src]++);
      CHECK(p.obs_point[src] == o.point_perm[i]);
      const int f = p.obs_frame[src], b = t.fb[f];
      if (d > o.poff[i]) CHECK(t.fb[p.obs_frame[o.obs_perm[d - 1]]] <= b);   // constant frames (-1) first
      CHECK(o.obs_frame[d] == f && o.obs_pt[2 * d] == p.obs_pt[2 * src] && o.obs_pt[2 * d + 1] == p.obs_pt[2 * src + 1]);
      const int m = o.obs_meta[d];
      const bool pf = p.point_free[p.obs_point[src]] != 0;
      const bool fixed = b < 0 && !pf && !p.cameras_free;
      CHECK(meta_block(m) == b && meta_cam(m) == p.frame_camera[f]);
      CHECK(!!(m & kMetaRot) == !!p.frame_rot_free[f] && !!(m & kMetaTrans) == !!p.frame_trans_free[f]);
      CHECK(!!(m & kMetaPfree) == pf && !!(m & kMetaFixed) == fixed && !!o.obs_fixed[d] == fixed);
    }
}

// block of a device-order observation
static int Blk(const Truth& t, const Order& o, int d) { return t.fb[o.obs_frame[d]]; }

static void CheckSweep(const Truth& t, const Order& o, const WorkLists& w, int ncu, int knob) {
  const int P = o.P;
  CHECK(w.nlin == (int)w.lchunks.size());
  CHECK(w.lin_waves == (knob ? knob : (2LL * w.nlin <= 12LL * ncu ? 2 : 1)));
  int pnext = 0, rnext = 0, cam = 0;
  std::multiset<int> units(w.pu_units.begin(), w.pu_units.begin() + w.npu);
  CHECK((int)w.pu_units.size() == std::max(w.npu, 1));
  int unext = 0;
  for (int c = 0; c < w.nlin; ++c) {
    const LinChunk& ch = w.lchunks[c];
    CHECK(ch.p0 == pnext && ch.p1 > ch.p0 && ch.p1 <= P);   // chunks partition [0, P)
    CHECK(ch.r0 == rnext && ch.r1 > ch.r0 && ch.r1 <= (int)w.lrounds.size());
    if (ch.p1 <= ch.p0 || ch.p1 > P || ch.r1 > (int)w.lrounds.size()) return;
    pnext = ch.p1;
    rnext = ch.r1;
    CHECK(ch.cam_off == cam);   // running sum of nb * kCamV
    cam += ch.nb * kCamV;
    CHECK(ch.u0 == unext);
    int onext = o.poff[ch.p0];   // rounds partition the chunk's observations
    for (int r = ch.r0; r < ch.r1; ++r) {
      CHECK(w.lrounds[r].o0 == onext && w.lrounds[r].o1 >= onext);
      onext = w.lrounds[r].o1;
    }
    CHECK(onext == o.poff[ch.p1]);
    if (ch.wide) {
      CHECK(ch.p1 == ch.p0 + 1);
      const int i = ch.p0, kobs = o.poff[i + 1] - o.poff[i];
      const int span = t.last[o.point_perm[i]] < 0 ? 0 : t.last[o.point_perm[i]] - t.first[o.point_perm[i]] + 1;
      CHECK(kobs > kLinObs || span > kLinNbMax);
      for (int r = ch.r0; r < ch.r1; ++r) {   // pieces of the one point
        const LinRound& R = w.lrounds[r];
        CHECK(R.p0 == i && R.p1 == i + 1 && R.o1 - R.o0 <= kLinObs && R.o1 > R.o0);
      }
      CHECK(units.count(-(c + 1)) == 1 && w.pu_units[ch.u0] == -(c + 1));
      unext += 1;
      continue;
    }
    CHECK(ch.r1 - ch.r0 <= kLinMaxRounds);
    int rp = ch.p0;
    for (int r = ch.r0; r < ch.r1; ++r) {   // whole points
      const LinRound& R = w.lrounds[r];
      CHECK(R.p0 == rp && R.p1 > R.p0 && R.p1 <= ch.p1);
      if (R.p1 <= R.p0 || R.p1 > ch.p1) return;
      rp = R.p1;
      CHECK(R.o0 == o.poff[R.p0] && R.o1 == o.poff[R.p1]);
      CHECK(R.o1 - R.o0 <= kLinObs && R.p1 - R.p0 <= kLinPts);
      CHECK(units.count(r) == 1 && w.pu_units[ch.u0 + r - ch.r0] == r);
    }
    CHECK(rp == ch.p1);
    unext += ch.r1 - ch.r0;
    CHECK(ch.nb >= 0 && ch.nb <= kLinNbMax);
    int nconst = 0;
    for (int i = ch.p0; i < ch.p1; ++i) {
      nconst += t.last[o.point_perm[i]] < 0;
      for (int d = o.poff[i]; d < o.poff[i + 1]; ++d) {
        const int b = Blk(t, o, d);
        if (b >= 0) CHECK(b >= ch.b_lo && b < ch.b_lo + ch.nb);
      }
    }
    CHECK(nconst == 0 || nconst == ch.p1 - ch.p0);   // constant-only points are not mixed with others
    if (nconst) CHECK(ch.nb == 0);
  }
  CHECK(pnext == P && rnext == (int)w.lrounds.size() && cam == w.lcam_off && unext == w.npu);
}

static void CheckSchur(const Truth& t, const Order& o, const WorkLists& w) {
  const int P = o.P;
  // the Schur span of a point: a free point's blocks [first, last]
  auto span = [&](int i) {
    const int pt = o.point_perm[i];
    return (o.pfree[i] && t.last[pt] >= 0) ? t.last[pt] - t.first[pt] + 1 : 0;
  };
  auto first = [&](int i) { return t.first[o.point_perm[i]]; };
  CHECK((int)w.segs.size() == std::max(w.nseg, 1) && (int)w.wsegs.size() == std::max(w.nwide, 1));
  CHECK((int)w.pinfo.size() == 2 * std::max(P, 1) && (int)w.pmx.size() == 4 * std::max(P, 1));
  // segments and wide segments cover every point once, in order
  std::vector<int> cover(P, 0);
  int pprev = 0, bnext = 0, cnext = 0;
  std::vector<std::pair<int, int>> slabs;
  size_t npairs = 0;
  for (int i = 0; i < P; ++i) {
    size_t kb = 0;
    for (int d = o.poff[i]; d < o.poff[i + 1]; ++d) kb += Blk(t, o, d) >= 0;
    if (o.pfree[i]) npairs += kb * (kb + 1) / 2;
  }
  CHECK(npairs == w.npairs);
  for (int s = 0; s < w.nseg; ++s) {
    const SchurSeg& sg = w.segs[s];
    CHECK(sg.p0 >= pprev && sg.p1 > sg.p0 && sg.p1 <= P);
    if (sg.p1 <= sg.p0 || sg.p0 < 0 || sg.p1 > P) return;
    pprev = sg.p1;
    CHECK(sg.ntw >= 0 && sg.ntw <= kSchurTW);
    const int ntile = sg.ntw * (sg.ntw + 1) / 2;
    slabs.emplace_back(sg.s_off, sg.s_off + 256 * ntile + 16 * sg.ntw);
    CHECK(sg.bt0 == bnext && sg.bt1 >= sg.bt0 && sg.bt1 <= (int)w.sbatch.size());
    if (sg.bt1 > (int)w.sbatch.size()) return;
    bnext = sg.bt1;
    int kp = sg.p0;
    for (int b = sg.bt0; b < sg.bt1; ++b) {
      const SchurBatch& B = w.sbatch[b];
      CHECK(B.p0 == kp && B.p1 > B.p0 && B.p1 <= sg.p1);
      if (B.p1 <= B.p0 || B.p1 > sg.p1) return;
      kp = B.p1;
      CHECK(B.c0 == cnext && B.c1 >= B.c0);   // cell ranges are contiguous
      CHECK(B.p1 - B.p0 <= kSchurBatchPts && B.c1 - B.c0 <= 64 * kSchurCellWaves);
      int nx = 0, nc = 0;
      for (int i = B.p0; i < B.p1; ++i) {
        cover[i]++;
        const int sp = span(i);
        CHECK(sp <= kSegNbMax);
        const int jhi = sp == 0 ? -1 : (6 * (first(i) + sp) - 1) / 16 - sg.t0;
        CHECK(jhi < sg.ntw);   // the point ends inside the window
        if (sp) {
          CHECK(6 * first(i) / 16 >= sg.t0 && jhi >= 0);
          CHECK(first(i) >= sg.b_lo && first(i) + sp <= sg.b_lo + sg.nb);
          CHECK(o.pfree[i]);   // every celled point is free
        }
        CHECK(w.pmx[4 * i] == nx && w.pmx[4 * i + 1] == jhi && w.pmx[4 * i + 3] == nc);
        if (sp) CHECK(w.pinfo[2 * i] == B.c0 + nc && w.pinfo[2 * i + 1] == ((first(i) << 8) | sp));
        else CHECK(w.pinfo[2 * i] == 0 && w.pinfo[2 * i + 1] == 0);
        // its cells: the blocks [first, first + span), each with the point's observations in that block
        std::map<int, std::vector<int>> byblk;
        bool simple = sp > 0;
        int nfree = 0;
        for (int d = o.poff[i]; d < o.poff[i + 1]; ++d) {
          const int bb = Blk(t, o, d);
          if (bb < 0) continue;
          if (sp) byblk[bb].push_back(d);
          simple = simple && bb == first(i) + nfree && (nfree == 0 || Blk(t, o, d - 1) == bb - 1);
          ++nfree;
        }
        simple = simple && nfree == sp;
        int d0 = -1;
        for (int d = o.poff[i]; d < o.poff[i + 1] && d0 < 0; ++d)
          if (Blk(t, o, d) >= 0) d0 = d;
        CHECK(w.pmx[4 * i + 2] == (simple ? d0 : -1));   // simple_obs
        for (int q = 0; q < sp; ++q) {
          const size_t c = (size_t)B.c0 + nc + q;
          CHECK(4 * c + 3 < w.cells.size());
          if (4 * c + 3 >= w.cells.size()) return;
          const int32_t* cell = &w.cells[4 * c];
          const int bb = first(i) + q, more = cell[2] & 0xffff;
          CHECK(cell[1] == i && (cell[2] >> 16) == bb);
          std::vector<int> got;
          if (cell[0] >= 0) got.push_back(cell[0]);
          CHECK(cell[0] >= 0 || more == 0);
          CHECK(cell[3] >= 0 && (size_t)cell[3] + more <= w.cell_obs.size());
          if ((size_t)cell[3] + more > w.cell_obs.size()) return;
          for (int x = 0; x < more; ++x) got.push_back(w.cell_obs[cell[3] + x]);
          std::sort(got.begin(), got.end());
          CHECK(got == byblk[bb]);
        }
        nx += 64 * (jhi + 1);
        nc += sp;
      }
      CHECK(nx <= kSchurXCap && nc == B.c1 - B.c0);
      cnext = B.c1;
    }
    CHECK(kp == sg.p1);
  }
  CHECK(cnext == w.ncell && bnext == (w.nseg ? (int)w.sbatch.size() : 0));
  CHECK(w.cells.size() == 4 * (size_t)std::max(w.ncell, 1));
  int wprev = -1;
  size_t pnext = 0;
  for (int k = 0; k < w.nwide; ++k) {
    const WideSeg& ws = w.wsegs[k];
    CHECK(ws.p > wprev && ws.p < P);
    if (ws.p <= wprev || ws.p >= P) return;
    wprev = ws.p;
    cover[ws.p]++;
    CHECK(span(ws.p) > kSegNbMax && o.pfree[ws.p]);
    CHECK((size_t)ws.pair_lo == pnext && ws.pair_hi >= ws.pair_lo && 2 * (size_t)ws.pair_hi <= w.pairs.size());
    if (2 * (size_t)ws.pair_hi > w.pairs.size()) return;
    pnext = ws.pair_hi;
    std::vector<std::pair<int, int>> want, got;
    const int o0 = o.poff[ws.p];
    for (int a = o0; a < o.poff[ws.p + 1]; ++a)
      for (int b = a; b < o.poff[ws.p + 1]; ++b)
        if (Blk(t, o, a) >= 0 && Blk(t, o, b) >= 0)
          want.emplace_back(((a - o0) << 16) | (b - o0), (Blk(t, o, a) << 16) | Blk(t, o, b));
    for (int x = ws.pair_lo; x < ws.pair_hi; ++x) got.emplace_back(w.pairs[2 * x], w.pairs[2 * x + 1]);
    std::sort(want.begin(), want.end());
    std::sort(got.begin(), got.end());
    CHECK(want == got);
  }
  for (int i = 0; i < P; ++i) {
    CHECK(cover[i] == 1);
    CHECK((span(i) > kSegNbMax) == (std::binary_search(w.wsegs.begin(), w.wsegs.begin() + w.nwide, WideSeg{i, 0, 0, 0},
                                                       [](const WideSeg& a, const WideSeg& b) { return a.p < b.p; })));
  }
  std::sort(slabs.begin(), slabs.end());   // s_off ranges do not overlap
  int send = 0;
  for (const auto& sl : slabs) {
    CHECK(sl.first >= send);
    send = sl.second;
  }
  CHECK(send <= w.s_off);
}

static void CheckReduceLists(const Order& o, const WorkLists& w, const Envelope& e) {
  const int NB = o.NB;
  CHECK((int)w.cam_loff.size() == NB + 1 && (int)w.r_loff.size() == NB + 1);
  CHECK(w.r_lstride % 256 == 0 && w.r_lstride >= 256 && e.s_lstride % 256 == 0 && e.s_lstride >= 256);
  CHECK(w.r_lidx.size() == (size_t)std::max(NB, 1) * w.r_lstride);
  for (int b = 0; b < NB; ++b) {
    std::vector<int> want;   // every covering chunk once, in chunk order
    for (const LinChunk& ch : w.lchunks)
      if (!ch.wide && b >= ch.b_lo && b < ch.b_lo + ch.nb) {
        want.push_back(ch.cam_off + (b - ch.b_lo) * kCamV);
        CHECK(want.back() + kCamV <= w.lcam_off);
      }
    CHECK(w.cam_loff[b + 1] - w.cam_loff[b] == (int)want.size() && w.cam_loff[b + 1] <= (int)w.cam_lidx.size());
    if (w.cam_loff[b + 1] > (int)w.cam_lidx.size()) return;
    CHECK(std::equal(want.begin(), want.end(), w.cam_lidx.begin() + w.cam_loff[b]));
    want.clear();
    for (int s = 0; s < w.nseg; ++s) {
      const SchurSeg& sg = w.segs[s];
      if (b < sg.b_lo || b >= sg.b_lo + sg.nb) continue;
      const int off = sg.s_off + 256 * (sg.ntw * (sg.ntw + 1) / 2) + 6 * b - 16 * sg.t0;
      CHECK(6 * b - 16 * sg.t0 >= 0 && 6 * b - 16 * sg.t0 + 6 <= 16 * sg.ntw);   // inside the segment's rhs
      want.push_back(off);
    }
    CHECK(w.r_loff[b] == (int)want.size() && (int)want.size() <= w.r_lstride);
    CHECK(std::equal(want.begin(), want.end(), w.r_lidx.begin() + (size_t)b * w.r_lstride));
  }
  // the band tiles of the frame columns, and per tile exactly the segment tiles that cover it
  const int nft = (6 * NB + kCholNb - 1) / kCholNb;
  std::vector<int> tiles;
  for (int R = 0; R < nft; ++R)
    for (int C = R; C < std::min(nft, (e.panel_jmax[R] + kCholNb - 1) / kCholNb); ++C) tiles.push_back((R << 16) | C);
  CHECK(e.nstile == (int)tiles.size() && (int)e.stile.size() == std::max(e.nstile, 1));
  CHECK((int)e.s_loff.size() == std::max(e.nstile, 1) && e.s_lidx.size() == (size_t)std::max(e.nstile, 1) * e.s_lstride);
  if (e.nstile != (int)tiles.size()) return;
  for (int x = 0; x < e.nstile; ++x) {
    CHECK(e.stile[x] == tiles[x]);
    const int R = tiles[x] >> 16, C = tiles[x] & 0xffff;
    std::vector<int> want;
    for (int s = 0; s < w.nseg; ++s) {
      const SchurSeg& sg = w.segs[s];
      const int r = R - sg.t0, c = C - sg.t0;
      if (r >= 0 && c < sg.ntw) want.push_back(sg.s_off + 256 * (c * (c + 1) / 2 + r));   // (+ 256 <= the rhs part)
    }
    CHECK(e.s_loff[x] == (int)want.size() && (int)want.size() <= e.s_lstride);
    CHECK(std::equal(want.begin(), want.end(), e.s_lidx.begin() + (size_t)x * e.s_lstride));
  }
}

static void CheckEnvelope(const sg_problem& p, const Truth& t, const Order& o, const Envelope& e) {
  const int n = o.n, NB = o.NB, npanel = (n + kCholNb - 1) / kCholNb;
  CHECK(e.npanel == npanel && (int)e.panel_jmax.size() == std::max(npanel, 1) * (o.nk ? 2 : 1));
  CHECK((int)e.pack_off.size() == npanel + 1 && e.pack_off[0] == 0);
  int bt = 0;
  for (int pk = 0; pk < npanel; ++pk) {
    const int j = e.panel_jmax[pk];
    CHECK((j % kCholNb == 0 || j == n) && j <= n && j >= std::min(n, (pk + 1) * kCholNb));
    if (o.nk) {   // dense through the intrinsics columns; the frame band ends follow as a tail
      CHECK(j == n);
      const int be = e.panel_jmax[npanel + pk];
      CHECK(be <= 6 * NB && be >= std::min(6 * NB, (pk + 1) * kCholNb));
    }
    CHECK(e.pack_off[pk + 1] == e.pack_off[pk] + std::min(kCholNb, n - pk * kCholNb) * (j - pk * kCholNb));
    bt = std::max(bt, (j + kCholNb - 1) / kCholNb - pk);
  }
  CHECK(e.npack == (size_t)e.pack_off[npanel] + n && e.band_tiles == bt);
  // every coupled block pair I <= J: the columns of J lie below the band end of every panel holding rows of I
  auto covered = [&](int I, int J) {
    for (int pk = 6 * I / kCholNb; pk <= (6 * I + 5) / kCholNb; ++pk) {
      CHECK(6 * J + 6 <= e.panel_jmax[pk]);
      if (o.nk) CHECK(6 * J + 6 <= (e.panel_jmax[npanel + pk] + kCholNb - 1) / kCholNb * kCholNb);
    }
  };
  for (int i = 0; i < p.num_points; ++i) {
    if (!p.point_free[i]) continue;
    std::set<int> blocks;
    for (int ob : t.pobs[i])
      if (t.fb[p.obs_frame[ob]] >= 0) blocks.insert(t.fb[p.obs_frame[ob]]);
    for (int I : blocks)
      for (int J : blocks)
        if (I <= J) covered(I, J);
  }
  for (int d = 0; d < p.num_dist; ++d) {
    const int a = t.fb[p.dist_frame[d]], b = t.fb[p.dist_prev[d]];
    if (a >= 0 && b >= 0) covered(std::min(a, b), std::max(a, b));
  }
}

static void CheckFrameDistance(const sg_problem& p, const Truth& t, const Order& o, const WorkLists& w) {
  const int NB = o.NB, D = p.num_dist;
  CHECK((int)w.fd_a.size() == std::max(D, 1) && (int)w.fd_b.size() == std::max(D, 1));
  CHECK((int)w.fd_boff.size() == NB + 1 && w.fd_pair.size() == (size_t)std::max(NB, 1) * std::max(NB, 1));
  std::vector<std::vector<int>> lists(NB);
  std::vector<int> pair((size_t)std::max(NB, 1) * std::max(NB, 1), -1);
  for (int d = 0; d < D; ++d) {
    CHECK(w.fd_a[d] == p.dist_frame[d] && w.fd_b[d] == p.dist_prev[d]);
    const int a = t.fb[p.dist_frame[d]], b = t.fb[p.dist_prev[d]];
    if (a >= 0) lists[a].push_back(2 * d);
    if (b >= 0) lists[b].push_back(2 * d + 1);
    if (a >= 0 && b >= 0 && a != b) pair[(size_t)std::min(a, b) * NB + std::max(a, b)] = 2 * d + (a < b ? 0 : 1);
  }
  CHECK(std::equal(pair.begin(), pair.end(), w.fd_pair.begin()));
  for (int b = 0; b < NB; ++b) {
    CHECK(w.fd_boff[b + 1] - w.fd_boff[b] == (int)lists[b].size() && w.fd_boff[b + 1] <= (int)w.fd_bidx.size());
    if (w.fd_boff[b + 1] > (int)w.fd_bidx.size()) return;
    CHECK(std::equal(lists[b].begin(), lists[b].end(), w.fd_bidx.begin() + w.fd_boff[b]));
  }
  if (!o.nk) return;
  // free intrinsics: per frame block (then block NB: the fixed frames') its non-fixed observations, in order
  CHECK((int)w.intr_boff.size() == NB + 2);
  int lmax = 1;
  for (int b = 0; b <= NB; ++b) {
    std::vector<int> want;
    for (int d = 0; d < o.M; ++d)
      if (!(o.obs_meta[d] & kMetaFixed) && (Blk(t, o, d) >= 0 ? Blk(t, o, d) : NB) == b) want.push_back(d);
    CHECK(w.intr_boff[b + 1] - w.intr_boff[b] == (int)want.size() && w.intr_boff[b + 1] <= (int)w.intr_bidx.size());
    if (w.intr_boff[b + 1] > (int)w.intr_bidx.size()) return;
    CHECK(std::equal(want.begin(), want.end(), w.intr_bidx.begin() + w.intr_boff[b]));
    lmax = std::max(lmax, (int)want.size());
  }
  CHECK(!w.intr_bidx.empty() && w.intr_nsl == std::max(1, std::min(32, (lmax + 255) / 256)));
}

static Plan CheckAll(const char* name, Prob* pr, int ncu = 256, const LoadKnobs& k = LoadKnobs()) {
  g_case = name;
  const sg_problem p = pr->view();
  const Truth t = MakeTruth(p);
  Plan pl = MakePlan(p, ncu, k);
  CheckOrder(p, t, pl.o);
  CheckSweep(t, pl.o, pl.w, ncu, k.lin_waves);
  CheckSchur(t, pl.o, pl.w);
  CheckReduceLists(pl.o, pl.w, pl.e);
  CheckEnvelope(p, t, pl.o, pl.e);
  CheckFrameDistance(p, t, pl.o, pl.w);
  printf("[%s] F %d P %d M %d NB %d n %d: chunks %d rounds %d units %d waves %d, segments %d batches %d wide %d "
         "cells %d, panels %d band tiles %d stiles %d\n", name, pl.o.F, pl.o.P, pl.o.M, pl.o.NB, pl.o.n, pl.w.nlin,
         (int)pl.w.lrounds.size(), pl.w.npu, pl.w.lin_waves, pl.w.nseg, (int)pl.w.sbatch.size(), pl.w.nwide,
         pl.w.ncell, pl.e.npanel, pl.e.band_tiles, pl.e.nstile);
  return pl;
}

static const CholGrants kGrants{128 * 1024, 128 * 1024, 128 * 1024};
static CholPlan Chol(const char* name, const Plan& pl, const LoadKnobs& k, const CholGrants& g = kGrants) {
  g_case = name;
  const CholPlan c = PlanChol(pl.o, pl.e, g, k);
  printf("[%s] cholesky: tiles %d border %d (flags %d) window %d gstage %d cand_lds %d nd %d ns %d lds %zu wg %zu\n",
         name, c.tiles, c.border, c.border_flags, c.window, c.gstage, c.cand_lds, c.nd, c.ns, c.tile_lds, c.wg_size);
  return c;
}
// every panel's band fits k_cholesky_window's LDS window
static bool FitsWindow(const Plan& pl) {
  bool fits = pl.e.npanel <= kJendSh;
  for (int pk = 0; pk < pl.e.npanel; ++pk) fits = fits && pl.e.panel_jmax[pk] - pk * kCholNb <= kCholWS;
  return fits;
}

int main() {
  Rng rng{20240611};
  {   // (a) the plain case: n = 102, 7 tile rows, below kSplitMinNT
    Prob pr = MakeFrames(20, 3, true);
    AddRandomPoints(&pr, &rng, 400, 2, 8, 0, 20);
    Finish(&pr, &rng);
    const Plan pl = CheckAll("a", &pr);
    CHECK(pl.o.n == 102 && pl.e.npanel == 7 && pl.e.npanel < kSplitMinNT);
    const CholPlan c = Chol("a", pl, LoadKnobs());
    CHECK(c.tiles && !c.border && c.nd == 0 && c.wg_size > 0);
    // few CUs: long segments, so the batch caps (points, operand doubles, cells) bind
    const Plan p4 = CheckAll("a ncu=4", &pr, 4);
    CHECK((int)p4.w.sbatch.size() > p4.w.nseg);
    g_case = "a lin_waves=1";
    LoadKnobs k1;
    k1.lin_waves = 1;
    CHECK(MakePlan(pr.view(), 256, k1).w.lin_waves == 1);
  }
  {   // (b) wide points (span > kSegNbMax) and a point with more than kLinObs observations
    Prob pr = MakeFrames(70, 4, true);
    AddRandomPoints(&pr, &rng, 300, 2, 10, 0, 70);
    for (int i = 0; i < 3; ++i) AddPoint(&pr, 10 + 12 * i, 30, true);
    AddPoint(&pr, 0, 70, true);
    Finish(&pr, &rng);
    const Plan pl = CheckAll("b", &pr);
    CHECK(pl.w.nwide == 4);
    int wide_chunks = 0, pieces = 0;
    for (const LinChunk& ch : pl.w.lchunks)
      if (ch.wide) {
        ++wide_chunks;
        pieces = std::max(pieces, ch.r1 - ch.r0);
      }
    CHECK(wide_chunks == 4 && pieces == 2);   // 70 observations: two pieces of one point
    Chol("b", pl, LoadKnobs());
  }
  {   // (c) 15 tile rows, bands within kTB tiles: the dissected band
    Prob pr = MakeFrames(44, 4, true);
    AddRandomPoints(&pr, &rng, 600, 2, 8, 0, 44);
    Finish(&pr, &rng);
    const Plan pl = CheckAll("c", &pr);
    const int nt = pl.e.npanel;
    CHECK(pl.o.n == 240 && nt == 15 && pl.e.band_tiles <= kTB);
    const CholPlan c = Chol("c default", pl, LoadKnobs());
    CHECK(c.tiles && !c.border && c.nd >= 2 && c.ns >= 1 && c.ns <= 7 && nt - c.nd - c.ns >= 1);
    {   // (m, ns, nd) attains the minimum of max(m, nd + 2.5) + ns over the feasible set
      double best = 1e30;
      for (int m = 1; m < nt; ++m)
        for (int ns = 1; ns <= kTB - 1; ++ns) {
          const int nd = nt - m - ns;
          int reach = 0;   // the separator holds every band of the top part
          for (int K = 0; K < m; ++K) reach = std::max(reach, std::min(nt, (pl.e.panel_jmax[K] + kCholNb - 1) / kCholNb));
          if (nd < 2 || reach - m > ns) continue;
          best = std::min(best, std::max((double)m, nd + 2.5) + ns);
        }
      const int m = nt - c.nd - c.ns;
      CHECK(std::max((double)m, c.nd + 2.5) + c.ns == best);
      int reach = 0;
      for (int K = 0; K < m; ++K) reach = std::max(reach, std::min(nt, (pl.e.panel_jmax[K] + kCholNb - 1) / kCholNb));
      CHECK(reach - m <= c.ns);
    }
    LoadKnobs k7;
    k7.chol_sep7 = true;
    const CholPlan c7 = Chol("c sep=7", pl, k7);
    CHECK(c7.tiles && c7.ns == 7 && c7.nd == (nt - 9) / 2);
    LoadKnobs k0;
    k0.chol_split = false;
    const CholPlan c0 = Chol("c split off", pl, k0);
    CHECK(c0.tiles && c0.nd == 0);
    // (e) the k_chol_tiles grant at 1 KiB: the one-workgroup kernels
    const CholPlan c1 = Chol("c 1 KiB grant", pl, LoadKnobs(), CholGrants{1024, 128 * 1024, 128 * 1024});
    CHECK(!c1.tiles && !c1.border && c1.nd == 0);
    LoadKnobs kw;
    kw.chol_window = true;
    const CholPlan cw = Chol("c window knob", pl, kw);
    CHECK(!cw.tiles && cw.nd == 0 && cw.window == FitsWindow(pl));
  }
  {   // (d) free intrinsics, nk = 7: the bordered band, and with the border knob off the one-workgroup kernels
    Prob pr = MakeFrames(10, 2, true);
    pr.cameras_free = 1;
    AddRandomPoints(&pr, &rng, 120, 2, 6, 0, 10);
    Finish(&pr, &rng);
    const Plan pl = CheckAll("d", &pr);
    CHECK(pl.o.nk == 7 && pl.o.n == 55);
    const CholPlan c = Chol("d border", pl, LoadKnobs());
    CHECK(c.border && c.tiles && c.nd == 0 && c.border_flags >= 1 && c.border_flags <= 3);
    LoadKnobs kb;
    kb.chol_border = false;
    const CholPlan cg = Chol("d border off", pl, kb);
    // S (n = 55) fits k_cholesky_window's LDS window, which takes it before k_cholesky_global does
    CHECK(!cg.border && !cg.tiles && cg.nd == 0 && cg.window == FitsWindow(pl));
  }
  {   // (d2) free intrinsics past kCholWS columns: with the border knob off, k_cholesky_global
    Prob pr = MakeFrames(26, 2, true);
    pr.cameras_free = 1;
    AddRandomPoints(&pr, &rng, 200, 2, 6, 0, 26);
    Finish(&pr, &rng);
    const Plan pl = CheckAll("d2", &pr);
    CHECK(pl.o.n == 6 * 24 + 7 && pl.o.n > kCholWS);
    const CholPlan c = Chol("d2 border", pl, LoadKnobs());
    CHECK(c.border && c.tiles && c.border_flags >= 1 && c.border_flags <= 3);
    LoadKnobs kb;
    kb.chol_border = false;
    const CholPlan cg = Chol("d2 border off", pl, kb);
    CHECK(!cg.border && !cg.tiles && !cg.window && cg.gstage);
    kb.chol_gstage = false;
    CHECK(!Chol("d2 border off, unstaged", pl, kb).gstage);
  }
  {   // (e) points seen only from fixed frames, constant points on free frames, no FrameDistance
    Prob pr = MakeFrames(16, 4, false);
    AddRandomPoints(&pr, &rng, 150, 2, 8, 0, 16);
    AddRandomPoints(&pr, &rng, 20, 1, 4, 0, 4);   // fixed frames only
    for (int i = 0; i < 25; ++i) AddPoint(&pr, rng.range(2, 10), rng.range(2, 6), false);   // constant points
    Finish(&pr, &rng);
    const Plan pl = CheckAll("e", &pr);
    CHECK(pl.o.D == 0 && pl.w.fd_a.size() == 1 && pl.w.fd_bidx.size() == 1);
    Chol("e", pl, LoadKnobs());
  }
  {   // (e) every frame fixed: NB = 0, n = 0; every uploaded list still holds an element
    Prob pr = MakeFrames(6, 6, true);
    AddRandomPoints(&pr, &rng, 40, 2, 5, 0, 6);
    Finish(&pr, &rng);
    const Plan pl = CheckAll("all fixed", &pr);
    CHECK(pl.o.NB == 0 && pl.o.n == 0 && pl.w.nseg >= 1 && pl.w.ncell == 0 && pl.e.nstile == 0);
    const Order& o = pl.o;
    const WorkLists& w = pl.w;
    const Envelope& e = pl.e;
    CHECK(!o.frame_block.empty() && !o.pfree.empty() && !o.poff.empty() && !o.obs_pt.empty() && !o.obs_frame.empty() &&
          !o.obs_fixed.empty() && !o.obs_meta.empty() && !o.X.empty());
    CHECK(!w.lchunks.empty() && !w.lrounds.empty() && !w.pu_units.empty() && !w.segs.empty() && !w.sbatch.empty() &&
          !w.wsegs.empty() && !w.pinfo.empty() && !w.pmx.empty() && !w.cells.empty() && !w.cell_obs.empty() &&
          !w.pairs.empty() && !w.cam_loff.empty() && !w.cam_lidx.empty() && !w.r_loff.empty() && !w.r_lidx.empty() &&
          !w.fd_a.empty() && !w.fd_b.empty() && !w.fd_boff.empty() && !w.fd_bidx.empty() && !w.fd_pair.empty());
    CHECK(!e.panel_jmax.empty() && !e.pack_off.empty() && !e.stile.empty() && !e.s_loff.empty() && !e.s_lidx.empty());
    const CholPlan c = Chol("all fixed", pl, LoadKnobs());
    CHECK(!c.tiles && !c.border && c.nd == 0 && c.wg_size == 0);
  }
  {   // no points, no observations at all
    Prob pr = MakeFrames(5, 2, true);
    Finish(&pr, &rng);
    const Plan pl = CheckAll("no points", &pr);
    CHECK(pl.w.nlin == 0 && pl.w.nseg == 0 && pl.o.obs_meta.size() == 1);
    Chol("no points", pl, LoadKnobs());
  }
  if (g_fail) {
    printf("%d checks failed\n", g_fail);
    return 1;
  }
  printf("ba_plan_check OK\n");
  return 0;
}
