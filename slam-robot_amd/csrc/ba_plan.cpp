// ba_plan.cpp — the host-only planner of a full sg_ba_load (ba_plan.h): the device order, the work lists of the
// sweep and Schur kernels, the deterministic reduce lists, the Cholesky envelope and the Cholesky kernel choice.
#include "ba_plan.h"

#include <algorithm>
#include <climits>
#include <utility>

#include "common.h"

namespace sg {

// ================================================================================================
// Order

void PlanBlocks(const sg_problem& p, Order* o) {
  o->F = p.num_frames;
  o->P = p.num_points;
  o->M = p.num_obs;
  o->D = p.num_dist;
  // camera blocks: every frame with a free rotation or translation
  o->frame_block.assign(o->F, -1);
  o->NB = 0;
  for (int f = 0; f < o->F; ++f)
    if (p.frame_rot_free[f] || p.frame_trans_free[f]) o->frame_block[f] = o->NB++;
  o->nk = p.cameras_free ? 7 * p.num_cameras : 0;
  o->n = 6 * o->NB + o->nk;   // frame columns, then the free intrinsics
}

void PlanPointOrder(const sg_problem& p, Order* o) {
  const int P = o->P, M = o->M, NB = o->NB;
  // point order: by first free block (points without free-frame observations last)
  std::vector<int32_t> pfirst(P, NB), plast(P, -1);
  for (int ob = 0; ob < M; ++ob) {
    const int pt = p.obs_point[ob], b = o->frame_block[p.obs_frame[ob]];
    if (b >= 0) {
      pfirst[pt] = std::min(pfirst[pt], b);
      plast[pt] = std::max(plast[pt], b);
    }
  }
  // stable counting sort on the key pfirst in [0, NB]
  o->point_perm.resize(P);
  o->inv_perm.resize(P);
  {
    std::vector<int32_t> bstart(NB + 2, 0);
    for (int i = 0; i < P; ++i) bstart[pfirst[i] + 1]++;
    for (int b = 0; b <= NB; ++b) bstart[b + 1] += bstart[b];
    for (int i = 0; i < P; ++i) {
      const int pos = bstart[pfirst[i]]++;
      o->point_perm[pos] = i;
      o->inv_perm[i] = pos;
    }
  }
  // the first / last free block of each point in device order (the work-list builders read them per point)
  o->dfirst.resize(P);
  o->dlast.resize(P);
  for (int i = 0; i < P; ++i) {
    o->dfirst[i] = pfirst[o->point_perm[i]];
    o->dlast[i] = plast[o->point_perm[i]];
  }
}

void PlanObservations(const sg_problem& p, Order* o) {
  const int F = o->F, P = o->P, M = o->M;
  const std::vector<int32_t>& frame_block = o->frame_block;
  const std::vector<int32_t>& inv_perm = o->inv_perm;
  // observations: CSR by device point order (stable in problem order)
  std::vector<int32_t>& poff = o->poff;
  poff.assign(P + 1, 0);
  for (int ob = 0; ob < M; ++ob) poff[inv_perm[p.obs_point[ob]] + 1]++;
  for (int i = 0; i < P; ++i) poff[i + 1] += poff[i];
  o->obs_perm.assign(M, 0);
  {
    std::vector<int32_t> fill(poff.begin(), poff.end() - 1);
    for (int ob = 0; ob < M; ++ob) o->obs_perm[fill[inv_perm[p.obs_point[ob]]]++] = ob;
    // within a point: observations of constant frames first, then by camera block (stable), so that a point
    // observed once in every block of its span finds the observation of block b at a fixed offset (k_schur)
    // (a stable insertion sort: a point has a handful of observations, and std::stable_sort allocates a
    // buffer per call)
    for (int i = 0; i < P; ++i) {
      int32_t* v = o->obs_perm.data() + poff[i];
      const int k = poff[i + 1] - poff[i];
      if (k > 64) {
        std::stable_sort(v, v + k, [&](int a, int b) {
          return frame_block[p.obs_frame[a]] < frame_block[p.obs_frame[b]];
        });
        continue;
      }
      for (int x = 1; x < k; ++x) {
        const int32_t ob = v[x];
        const int key = frame_block[p.obs_frame[ob]];
        int y = x - 1;
        while (y >= 0 && frame_block[p.obs_frame[v[y]]] > key) {
          v[y + 1] = v[y];
          --y;
        }
        v[y + 1] = ob;
      }
    }
  }
  o->obs_pt.resize(2 * (size_t)M);
  o->obs_frame.resize(M);
  o->obs_fixed.resize(M);
  o->pfree.resize(P);
  o->X.resize(4 * (size_t)P);
  for (int i = 0; i < P; ++i) {
    const int pt = o->point_perm[i];
    o->pfree[i] = p.point_free[pt];
    for (int a = 0; a < 4; ++a) o->X[4 * i + a] = p.X[4 * pt + a];
  }
  o->obs_meta.assign(std::max(M, 1), 0);
  // per frame: the frame part of the packed observation word
  std::vector<int32_t> fmeta(F);
  for (int f = 0; f < F; ++f)
    fmeta[f] = (frame_block[f] + 1) | (p.frame_camera[f] << kMetaCamShift) | (p.frame_rot_free[f] ? kMetaRot : 0) |
               (p.frame_trans_free[f] ? kMetaTrans : 0);
  for (int ob = 0; ob < M; ++ob) {
    const int src = o->obs_perm[ob], f = p.obs_frame[src];
    const bool pf = p.point_free[p.obs_point[src]] != 0;
    o->obs_pt[2 * ob] = p.obs_pt[2 * src];
    o->obs_pt[2 * ob + 1] = p.obs_pt[2 * src + 1];
    o->obs_frame[ob] = f;
    o->obs_fixed[ob] = frame_block[f] < 0 && !pf && !p.cameras_free;
    o->obs_meta[ob] = fmeta[f] | (pf ? kMetaPfree : 0) | (o->obs_fixed[ob] ? kMetaFixed : 0);
  }
}

// ================================================================================================
// Work lists

// k_linearize decomposition (see LinChunk): rounds of whole points (<= kLinObs observations), up to
// maxr rounds per chunk sharing one camera window; fewer rounds per chunk on small problems so that the
// grid still fills the chip.
void PlanSweep(const Order& o, int ncu, int lin_waves_knob, WorkLists* w) {
  const int P = o.P, M = o.M, NB = o.NB;
  const std::vector<int32_t>&poff = o.poff, &dfirst = o.dfirst, &dlast = o.dlast;
  std::vector<LinRound>& lrounds = w->lrounds;
  std::vector<LinChunk>& lchunks = w->lchunks;
  int lcam_off = 0;
  {
    int maxr = std::max(1, std::min(kLinMaxRounds, M / (kLinObs * 1024)));
    auto kobs = [&](int i) { return poff[i + 1] - poff[i]; };
    auto constonly = [&](int i) { return dfirst[i] >= NB; };
    auto pspan = [&](int i) { return constonly(i) ? 0 : dlast[i] - dfirst[i] + 1; };
    for (int i = 0; i < P;) {
      LinChunk c{};
      c.p0 = i;
      c.r0 = (int)lrounds.size();
      if (kobs(i) > kLinObs || pspan(i) > kLinNbMax) {
        c.wide = 1;
        for (int ob = poff[i]; ob < poff[i + 1]; ob += kLinObs)
          lrounds.push_back(LinRound{ob, std::min(ob + kLinObs, poff[i + 1]), i, i + 1});
        c.p1 = ++i;
      } else {
        const bool co = constonly(i);
        int lo = co ? 0 : dfirst[i], hi = co ? -1 : dlast[i];
        int j = i, nr = 0;
        LinRound R{poff[i], poff[i], i, i};
        while (j < P) {
          if (kobs(j) > kLinObs || pspan(j) > kLinNbMax || constonly(j) != co) break;
          int l2 = lo, h2 = hi;
          if (!co) {
            l2 = std::min(lo, dfirst[j]);
            h2 = std::max(hi, dlast[j]);
            if (h2 - l2 + 1 > kLinNbMax) break;
          }
          if (R.o1 - R.o0 + kobs(j) > kLinObs || R.p1 - R.p0 >= kLinPts) {
            if (nr + 1 >= maxr) break;
            lrounds.push_back(R);
            ++nr;
            R = LinRound{poff[j], poff[j], j, j};
          }
          R.o1 += kobs(j);
          R.p1 = j + 1;
          lo = l2;
          hi = h2;
          ++j;
        }
        lrounds.push_back(R);
        c.p1 = j;
        c.b_lo = lo;
        c.nb = co ? 0 : hi - lo + 1;
        i = j;
      }
      c.r1 = (int)lrounds.size();
      c.cam_off = lcam_off;
      lcam_off += c.nb * kCamV;
      lchunks.push_back(c);
    }
  }
  w->lcam_off = lcam_off;
  w->nlin = (int)lchunks.size();
  // two waves per chunk (its rounds split between them) while the doubled grid still fits the chip at three
  // waves per SIMD (k_linearize's occupancy): config 2's ~1.5 k chunks; one wave per chunk when there are more
  // chunks than that (config 5, the scaled sweep), where the second wave only adds the combine.  (A producer /
  // consumer split of a chunk's rounds over two waves was measured slower at config 5: DESIGN.md 8.)
  w->lin_waves = 2 * (long long)w->nlin <= 12LL * ncu ? 2 : 1;
  if (lin_waves_knob) w->lin_waves = lin_waves_knob == 2 ? 2 : 1;   // A/B and tests
  std::vector<int32_t>& pu_units = w->pu_units;   // k_point_update work units
  for (int c = 0; c < w->nlin; ++c) {
    lchunks[c].u0 = (int)pu_units.size();   // k_update_lin writes the units' scalars
    if (lchunks[c].wide)
      pu_units.push_back(-(c + 1));
    else
      for (int r = lchunks[c].r0; r < lchunks[c].r1; ++r) pu_units.push_back(r);
  }
  w->npu = (int)pu_units.size();
  if (pu_units.empty()) pu_units.push_back(0);
}

// Schur work lists (see SchurSeg): the cells of every free point (one per block of its span, with the
// point's observations in that block), segments of consecutive points whose columns fit kSchurTW tiles of
// S, their batches, and each wide point's observation pairs (s <= t, both on free frames).
void PlanSchur(const Order& o, int ncu, WorkLists* w) {
  const int P = o.P, M = o.M, NB = o.NB;
  const std::vector<int32_t>&poff = o.poff, &dfirst = o.dfirst, &dlast = o.dlast;
  const std::vector<uint8_t>& pfree = o.pfree;
  std::vector<int32_t>&pinfo = w->pinfo, &pmx = w->pmx, &cells = w->cells, &cell_obs = w->cell_obs;
  std::vector<SchurSeg>& segs = w->segs;
  std::vector<SchurBatch>& sbatch = w->sbatch;
  std::vector<WideSeg>& wsegs = w->wsegs;
  std::vector<int32_t>& pairs_flat = w->pairs;
  pinfo.assign(2 * (size_t)std::max(P, 1), 0);
  pmx.assign(4 * (size_t)std::max(P, 1), 0);
  int s_off = 0;
  std::vector<int32_t> obs_blk(M);
  for (int ob = 0; ob < M; ++ob) obs_blk[ob] = o.frame_block[o.obs_frame[ob]];
  // span in blocks of a free point's Schur terms (0: none)
  std::vector<int32_t> ssp(std::max(P, 1));
  for (int i = 0; i < P; ++i) ssp[i] = (pfree[i] && dfirst[i] < NB) ? dlast[i] - dfirst[i] + 1 : 0;
  auto sspan = [&](int i) { return ssp[i]; };
  std::vector<int32_t> simple_obs(std::max(P, 1), -1);   // observation of the first block if one per block
  int ncell = 0;
  w->npairs = 0;
  w->schur_mfma = 0.0;
  w->schur_rhs = 0.0;
  w->schur_useful = 0.0;
  {
    std::vector<std::pair<int, int>> bo;
    cells.reserve(4 * (size_t)M + 4);
    cell_obs.reserve((size_t)M / 4 + 1);
    for (int i = 0; i < P; ++i) {
      size_t kb = 0;
      for (int ob = poff[i]; ob < poff[i + 1]; ++ob) kb += obs_blk[ob] >= 0;
      if (pfree[i]) w->npairs += kb * (kb + 1) / 2;
      const int sp = sspan(i);
      if (sp == 0 || sp > kSegNbMax) continue;
      // load_Jp_scaled and cell_load (k_schur) read a celled point's scaled Jacobian: a free point's only
      SG_REQUIRE(pfree[i], SG_EINVAL, "a constant point has Schur cells");
      const int pf = dfirst[i];
      pinfo[2 * i] = (int)(cells.size() / 4);
      pinfo[2 * i + 1] = (pf << 8) | sp;
      bo.clear();
      for (int ob = poff[i]; ob < poff[i + 1]; ++ob)
        if (obs_blk[ob] >= 0) bo.emplace_back(obs_blk[ob], ob);
      if (!std::is_sorted(bo.begin(), bo.end())) std::sort(bo.begin(), bo.end());   // sorted at load already
      {
        bool one = (int)bo.size() == sp;   // observations sorted by block at load: consecutive
        for (int q = 0; one && q < sp; ++q) one = bo[q].first == pf + q && bo[q].second == bo[0].second + q;
        if (one) simple_obs[i] = bo[0].second;
      }
      size_t k = 0;
      for (int b = pf; b < pf + sp; ++b) {
        // {first observation or -1, point, (block << 16) | further observations, their offset in cell_obs}
        int o0 = -1;
        if (k < bo.size() && bo[k].first == b) o0 = bo[k++].second;
        const int k1 = (int)cell_obs.size();
        while (k < bo.size() && bo[k].first == b) cell_obs.push_back(bo[k++].second);
        cells.insert(cells.end(), {o0, i, (int)(((unsigned)b << 16) | (unsigned)(cell_obs.size() - k1)), k1});
      }
    }
    ncell = (int)cells.size() / 4;
    if (cells.empty()) cells.assign(4, 0);
    if (cell_obs.empty()) cell_obs.push_back(0);
  }
  {
    // Segments: one per CU (the workgroup's LDS holds one per CU; fewer, longer segments write fewer partial tiles
    // and keep the producer/consumer pipeline full: 256 / 384 / 512 / 768 / 1024 segments measured 35.9 / 46.5 /
    // 40.9 / 47.8 / 53.0 us at C2, profiles/r2 segs sweep), balanced by the work of the busiest MFMA wave rather
    // than by point count (round 5): a point costs its slots on that wave, ceil(schur_aug_base(jhi + 1) /
    // kSchurCWaves) with jhi its last tile in the segment's window, plus kSegPointCost for its fetch (the MFMA
    // waves are the bound once the producers are pipelined; 0 / 1 / 2 / 4 / 8 measured C5 k_schur 292 / 260 /
    // 245 / 238 / 244 us against 259 with equal point counts, profiles/r5_s1_schur_ab.log).  The cap starts at the
    // estimated total / CUs (each point's tiles counted from its own first tile) and is raised while the window
    // breaks push the count past the CUs: two passes at C2 and C5.
    constexpr int kSegMinPts = 16;      // small problems: no segment of a handful of points
    constexpr int kSegPointCost = 4;
    auto point_cost = [&](int j, int tile0) {
      const int sp = sspan(j);
      if (sp == 0) return kSegPointCost;
      const int e = (6 * (dfirst[j] + sp) - 1) / 16 - tile0;
      return kSegPointCost + (schur_aug_base(e + 1) + kSchurCWaves - 1) / kSchurCWaves;
    };
    std::vector<int32_t> seg_end;   // exclusive end of each planned segment, in point order
    auto plan = [&](long long cap) {
      seg_end.clear();
      for (int i = 0; i < P;) {
        if (sspan(i) > kSegNbMax) {   // a wide point: k_schur_wide (the build loop below)
          ++i;
          continue;
        }
        int clo = INT32_MAX, chi = -1, j = i;
        long long acc = 0;
        while (j < P) {
          const int sp = sspan(j);
          if (sp > kSegNbMax) break;
          int l2 = clo, h2 = chi;
          if (sp > 0) {
            const int pf = dfirst[j];
            l2 = std::min(clo, 6 * pf);
            h2 = std::max(chi, 6 * (pf + sp));
            if ((h2 + 15) / 16 - l2 / 16 > kSchurTW) break;
          }
          const int c = point_cost(j, l2 == INT32_MAX ? 0 : l2 / 16);
          if (j - i >= kSegMinPts && acc + c > cap) break;
          acc += c;
          clo = l2;
          chi = h2;
          ++j;
        }
        seg_end.push_back(j);
        i = j;
      }
    };
    {
      long long est = 0;
      for (int j = 0; j < P; ++j)
        if (sspan(j) <= kSegNbMax) est += point_cost(j, sspan(j) ? 6 * dfirst[j] / 16 : 0);
      long long cap = std::max(1LL, (est + ncu - 1) / ncu);
      for (int pass = 0; pass < 8; ++pass) {
        plan(cap);
        if ((int)seg_end.size() <= ncu) break;
        cap += cap * (seg_end.size() - ncu) * 3 / (2 * ncu) + cap / 200 + 1;
      }
    }
    size_t next_seg = 0;
    int cnext = 0;
    for (int i = 0; i < P;) {
      if (sspan(i) > kSegNbMax) {
        SG_REQUIRE(pfree[i], SG_EINVAL, "a constant point is a wide Schur segment");
        WideSeg ws{};
        ws.p = i;
        ws.pair_lo = (int)pairs_flat.size() / 2;
        for (int os = poff[i]; os < poff[i + 1]; ++os) {
          if (obs_blk[os] < 0) continue;
          for (int ot = os; ot < poff[i + 1]; ++ot) {
            if (obs_blk[ot] < 0) continue;
            pairs_flat.push_back(((os - poff[i]) << 16) | (ot - poff[i]));
            pairs_flat.push_back((obs_blk[os] << 16) | obs_blk[ot]);
          }
        }
        ws.pair_hi = (int)pairs_flat.size() / 2;
        wsegs.push_back(ws);
        ++i;
        continue;
      }
      SchurSeg sg{};
      sg.p0 = i;
      int clo = INT32_MAX, chi = -1, blo = INT32_MAX, bhi = -1;   // columns [clo, chi), blocks [blo, bhi]
      int j = i;
      SG_REQUIRE(next_seg < seg_end.size() && seg_end[next_seg] > i, SG_EINVAL, "Schur segment plan out of step");
      const int jend = seg_end[next_seg++];
      while (j < jend) {
        const int sp = sspan(j);
        if (sp > kSegNbMax) break;
        if (sp > 0) {
          const int pf = dfirst[j];
          const int l2 = std::min(clo, 6 * pf), h2 = std::max(chi, 6 * (pf + sp));
          if ((h2 + 15) / 16 - l2 / 16 > kSchurTW) break;
          clo = l2;
          chi = h2;
          blo = std::min(blo, pf);
          bhi = std::max(bhi, pf + sp - 1);
        }
        ++j;
      }
      sg.p1 = j;
      if (chi >= 0) {
        sg.t0 = clo / 16;
        sg.ntw = (chi + 15) / 16 - sg.t0;
        sg.b_lo = blo;
        sg.nb = bhi - blo + 1;
      }
      // k_schur's asm chain (schur_chain.h) is entered at an offset computed from a point's last window tile:
      // every point must end inside the window (jhi <= kSchurTW - 1)
      SG_REQUIRE(sg.ntw <= kSchurTW, SG_EINVAL, "Schur segment window wider than kSchurTW");
      sg.s_off = s_off;
      s_off += sg.ntw * (sg.ntw + 1) / 2 * 256 + 16 * sg.ntw;
      // last window tile of each point's columns (-1: no Schur terms)
      auto pjhi = [&](int k) {
        const int sp = sspan(k);
        return sp == 0 ? -1 : (6 * (dfirst[k] + sp) - 1 - 16 * sg.t0) / 16;
      };
      sg.bt0 = (int)sbatch.size();
      for (int k = i; k < j;) {
        SchurBatch B{};
        B.p0 = k;
        B.c0 = cnext;
        int nc = 0, nx = 0;
        while (k < j && k - B.p0 < kSchurBatchPts && nx + 64 * (pjhi(k) + 1) <= kSchurXCap &&
               nc + sspan(k) <= 64 * kSchurCellWaves) {
          SG_REQUIRE(pjhi(k) < sg.ntw, SG_EINVAL, "point ends outside its Schur segment window");
          pmx[4 * k] = nx;
          pmx[4 * k + 1] = pjhi(k);
          pmx[4 * k + 2] = simple_obs[k];
          pmx[4 * k + 3] = nc;
          nx += 64 * (pjhi(k) + 1);
          w->schur_mfma += schur_aug_base(pjhi(k) + 1) - (pjhi(k) + 1);   // window tiles (16x16x4)
          w->schur_rhs += pjhi(k) + 1;                                      // rhs slots (4x4x4, 4 blocks)
          if (pjhi(k) >= 0) {   // the slots that multiply the point's own tiles (the rest multiply zeros)
            const double nu = pjhi(k) - (6 * dfirst[k] - 16 * sg.t0) / 16 + 1;
            w->schur_useful += 2048.0 * nu * (nu + 1) / 2 + 512.0 * nu;
          }
          nc += sspan(k++);
        }
        B.p1 = k;
        B.c1 = B.c0 + nc;
        cnext += nc;
        sbatch.push_back(B);
      }
      sg.bt1 = (int)sbatch.size();
      segs.push_back(sg);
      i = j;
    }
    SG_REQUIRE(cnext == ncell, SG_EINVAL, "Schur cells out of step with the batches");
  }
  w->ncell = ncell;
  w->s_off = s_off;
  w->nseg = (int)segs.size();
  w->nwide = (int)wsegs.size();
  if (segs.empty()) segs.resize(1);
  if (sbatch.empty()) sbatch.resize(1);
  if (wsegs.empty()) wsegs.resize(1);
  if (pairs_flat.empty()) pairs_flat.assign(2, 0);
}

// deterministic reduction lists: for every camera block, the slab offsets of the chunk partials that cover
// it (fixed chunk order), and of the segments' rhs partials
void PlanReduceLists(const Order& o, WorkLists* w) {
  const int NB = o.NB;
  std::vector<int32_t>&cam_loff = w->cam_loff, &cam_lidx = w->cam_lidx, &r_loff = w->r_loff, &r_lidx = w->r_lidx;
  cam_loff.assign(NB + 1, 0);
  r_loff.assign(NB + 1, 0);
  std::vector<std::vector<int32_t>> cl(NB), rl(NB);
  for (const LinChunk& ch : w->lchunks) {
    if (ch.wide || ch.nb == 0) continue;
    for (int i = 0; i < ch.nb; ++i) cl[ch.b_lo + i].push_back(ch.cam_off + i * kCamV);
  }
  for (int s = 0; s < w->nseg; ++s) {   // rhs partial of block I: window columns 6 I - 16 t0 ..
    const SchurSeg& sg = w->segs[s];
    const int ntile = sg.ntw * (sg.ntw + 1) / 2;
    for (int i = 0; i < sg.nb; ++i)
      rl[sg.b_lo + i].push_back(sg.s_off + 256 * ntile + 6 * (sg.b_lo + i) - 16 * sg.t0);
  }
  size_t rmax = 0;
  for (int b = 0; b < NB; ++b) rmax = std::max(rmax, rl[b].size());
  w->r_lstride = (int)std::max<size_t>(256, (rmax + 255) / 256 * 256);   // rows padded (k_S_reduce's unbounded reads)
  r_lidx.assign((size_t)std::max(NB, 1) * w->r_lstride, 0);
  for (int b = 0; b < NB; ++b) {
    cam_loff[b + 1] = cam_loff[b] + (int)cl[b].size();
    cam_lidx.insert(cam_lidx.end(), cl[b].begin(), cl[b].end());
    r_loff[b] = (int)rl[b].size();
    std::copy(rl[b].begin(), rl[b].end(), r_lidx.begin() + (size_t)b * w->r_lstride);
  }
  if (cam_lidx.empty()) cam_lidx.push_back(0);
}

void PlanFrameDistance(const sg_problem& p, const Order& o, WorkLists* w) {
  const int NB = o.NB, D = o.D;
  const std::vector<int32_t>& frame_block = o.frame_block;
  std::vector<int32_t>&fd_a = w->fd_a, &fd_b = w->fd_b, &fd_boff = w->fd_boff, &fd_bidx = w->fd_bidx;
  fd_a.assign(p.dist_frame, p.dist_frame + D);
  fd_b.assign(p.dist_prev, p.dist_prev + D);
  fd_boff.assign(NB + 1, 0);
  {
    std::vector<std::vector<int32_t>> lists(NB);
    for (int dd = 0; dd < D; ++dd) {
      const int ba = frame_block[fd_a[dd]], bb = frame_block[fd_b[dd]];
      if (ba >= 0) lists[ba].push_back(2 * dd);
      if (bb >= 0) lists[bb].push_back(2 * dd + 1);
    }
    for (int b = 0; b < NB; ++b) {
      fd_boff[b + 1] = fd_boff[b] + (int)lists[b].size();
      fd_bidx.insert(fd_bidx.end(), lists[b].begin(), lists[b].end());
    }
  }
  // FrameDistance cross-block lookup for the on-the-fly assembly: fd_pair[I*NB+J] (I<J) = 2 * residual +
  // (1 if the residual's frame a is block J, not I), so k_S_reduce reads the orientation with the index
  // instead of two more dependent loads (fd_a, frame_block)
  w->fd_pair.assign((size_t)std::max(NB, 1) * std::max(NB, 1), -1);
  for (int dd = 0; dd < D; ++dd) {
    const int ba = frame_block[fd_a[dd]], bb = frame_block[fd_b[dd]];
    if (ba >= 0 && bb >= 0 && ba != bb)
      w->fd_pair[(size_t)std::min(ba, bb) * NB + std::max(ba, bb)] = 2 * dd + (ba < bb ? 0 : 1);
  }
  // padded to one entry: k_cam_finalize prefetches fd_a[0] / fd_b[0] beside LmState even when D = 0
  if (fd_a.empty()) fd_a.push_back(0);
  if (fd_b.empty()) fd_b.push_back(0);
  if (fd_bidx.empty()) fd_bidx.push_back(0);
}

// free intrinsics: each frame block's non-fixed observations (block NB: the fixed frames'), for k_intr_fk
void PlanIntrLists(const Order& o, WorkLists* w) {
  if (!o.nk) return;
  const int NB = o.NB, M = o.M;
  const std::vector<int32_t>& obs_meta = o.obs_meta;
  std::vector<int32_t>&boff = w->intr_boff, &bidx = w->intr_bidx;
  boff.assign(NB + 2, 0);
  for (int ob = 0; ob < M; ++ob)
    if (!(obs_meta[ob] & kMetaFixed)) {
      const int b = meta_block(obs_meta[ob]);
      boff[(b >= 0 ? b : NB) + 1] += 1;
    }
  for (int b = 0; b <= NB; ++b) boff[b + 1] += boff[b];
  bidx.assign(std::max(boff[NB + 1], 1), 0);
  std::vector<int32_t> fill(boff.begin(), boff.end() - 1);
  for (int ob = 0; ob < M; ++ob)
    if (!(obs_meta[ob] & kMetaFixed)) {
      const int b = meta_block(obs_meta[ob]);
      bidx[fill[b >= 0 ? b : NB]++] = ob;
    }
  // slices per block list: about one observation per thread of a k_intr_fk workgroup
  int lmax = 1;
  for (int b = 0; b <= NB; ++b) lmax = std::max(lmax, boff[b + 1] - boff[b]);
  w->intr_nsl = std::max(1, std::min(32, (lmax + 255) / 256));
}

// Cholesky panel envelopes: block column J's first nonzero block row lo(J), exact from the observations of
// each free point (pairs of blocks it couples) and the FrameDistance pairs
void PlanLoBlk(const Order& o, WorkLists* w) {
  const int NB = o.NB;
  std::vector<int32_t>& lo_blk = w->lo_blk;
  lo_blk.resize(NB);
  for (int b = 0; b < NB; ++b) lo_blk[b] = b;
  for (int i = 0; i < o.P; ++i) {
    if (o.dfirst[i] >= NB) continue;
    if (!o.pfree[i]) continue;
    const int lo = o.dfirst[i];
    for (int ob = o.poff[i]; ob < o.poff[i + 1]; ++ob) {
      const int b = o.frame_block[o.obs_frame[ob]];
      if (b >= 0) lo_blk[b] = std::min(lo_blk[b], lo);
    }
  }
  for (int dd = 0; dd < o.D; ++dd) {
    const int ba = o.frame_block[w->fd_a[dd]], bb = o.frame_block[w->fd_b[dd]];
    if (ba >= 0 && bb >= 0) {
      const int hi3 = std::max(ba, bb), lo3 = std::min(ba, bb);
      lo_blk[hi3] = std::min(lo_blk[hi3], lo3);
    }
  }
}

// ================================================================================================
// Envelope

Envelope PlanEnvelope(const Order& o, const std::vector<int32_t>& lo_blk, const std::vector<SchurSeg>& segs,
                      int nseg) {
  const int n = o.n, NB = o.NB, nk = o.nk;
  Envelope e;
  const int npanel = e.npanel = (n + kCholNb - 1) / kCholNb;
  std::vector<int32_t>& panel_jmax = e.panel_jmax;
  panel_jmax.assign(std::max(npanel, 1), 0);
  std::vector<int32_t> panel_bend(std::max(npanel, 1), 0);
  for (int pk = 0; pk < npanel; ++pk) {
    const int row_hi = std::min(n, (pk + 1) * kCholNb) - 1;   // last row of the panel
    const int blk_hi = row_hi / 6;
    int jmax = (pk + 1) * kCholNb;
    // columns j whose envelope starts at or before the panel's last row block
    for (int b = 0; b < NB; ++b)
      if (lo_blk[b] <= blk_hi) jmax = std::max(jmax, 6 * b + 6);
    jmax = std::min(jmax, n);
    panel_jmax[pk] = std::min(n, (jmax + kCholNb - 1) / kCholNb * kCholNb);   // band end, 16-aligned
    if (nk) {   // the intrinsics columns couple every frame: S is dense (k_cholesky_global: arrowhead)
      panel_bend[pk] = std::min(jmax, 6 * NB);
      panel_jmax[pk] = n;
    }
  }
  if (nk) panel_jmax.insert(panel_jmax.end(), panel_bend.begin(), panel_bend.end());   // work_i_ tail
  e.pack_off.assign(npanel + 1, 0);
  for (int pk = 0; pk < npanel; ++pk)
    e.pack_off[pk + 1] = e.pack_off[pk] + std::min(kCholNb, n - pk * kCholNb) * (panel_jmax[pk] - pk * kCholNb);
  e.npack = (size_t)e.pack_off[npanel] + n;
  e.band_tiles = 0;
  for (int pk = 0; pk < npanel; ++pk)
    e.band_tiles = std::max(e.band_tiles, (panel_jmax[pk] + kCholNb - 1) / kCholNb - pk);
  // k_S_reduce work: the band tiles (R <= C) of the frame columns, and per tile the segment tiles covering it
  // (segment order).  A segment tile outside the band is zero (no point couples its rows and columns).
  std::vector<int32_t>&stile = e.stile, &s_loff = e.s_loff, &s_lidx = e.s_lidx;
  const int nft = (6 * NB + kCholNb - 1) / kCholNb;
  std::vector<int32_t> row_off(nft + 1, 0), cend(nft, 0);
  for (int R = 0; R < nft; ++R) {
    cend[R] = std::min(nft, (panel_jmax[R] + kCholNb - 1) / kCholNb);
    row_off[R + 1] = row_off[R] + std::max(0, cend[R] - R);
    for (int C = R; C < cend[R]; ++C) stile.push_back((R << 16) | C);
  }
  std::vector<std::vector<int32_t>> tl(stile.size());
  for (int s = 0; s < nseg; ++s) {
    const SchurSeg& sg = segs[s];
    for (int u = 0; u < sg.ntw * (sg.ntw + 1) / 2; ++u) {
      const int R = sg.t0 + schur_tile_r(u), C = sg.t0 + schur_tile_c(u);
      if (R < nft && C < cend[R]) tl[row_off[R] + C - R].push_back(sg.s_off + 256 * u);
    }
  }
  size_t smax = 0;
  for (const auto& l : tl) smax = std::max(smax, l.size());
  e.s_lstride = (int)std::max<size_t>(256, (smax + 255) / 256 * 256);   // rows padded (k_S_reduce's unbounded reads)
  s_lidx.assign(std::max<size_t>(tl.size(), 1) * e.s_lstride, 0);
  for (size_t t = 0; t < tl.size(); ++t) {
    s_loff.push_back((int)tl[t].size());
    std::copy(tl[t].begin(), tl[t].end(), s_lidx.begin() + t * e.s_lstride);
  }
  e.nstile = (int)stile.size();
  if (stile.empty()) stile.push_back(0);
  if (s_loff.empty()) s_loff.push_back(0);
  return e;
}

// ================================================================================================
// Cholesky choice

// The dissected band's hand-off, in phases of the top workgroup's chain: what the bottom workgroup takes beyond its
// nd phases before the top's separator waves see its signal.  Fitted from the hand-off stamps
// (profiles/chol_handoff_ab.log): at C2 (m = 7, nd = 6) the top's chain wave waits 1.14 - 1.27 of its phases at the
// poll of phase m - 1, so nd + h = m + 1.14 .. 1.27 and h = 2.14 .. 2.27, to a quarter phase 2.25 (2.5 before the write-through
// publish, when the wait was 1.5 phases).  The bottom's own phases were the longer ones (its tiles were loaded
// transposed), which h carried too.
// With the tiles read from St (PlanStile; profiles/chol_stile_ab.log) the wait at C2 is 6.2 - 6.7 k cycles of a 9.3 k
// phase, h = 1.67 - 1.72, to a quarter phase 1.75.  The price stays at 2.25 all the same.  Half a phase less on the
// bottom's side lowers no candidate by more than 0.5, so C2's split (13.25 now, 12.75 then) stays the cheapest, and
// C5 takes m = 35 at either price; but the fixed 7-row separator of the tests (SG_CHOL_SEP=7) is pinned to
// nd = (NT - 9) / 2, which at C2's 18 tile rows needs h > 2.
constexpr double kHandoffPhases = 2.25;

CholPlan PlanChol(const Order& o, const Envelope& e, const CholGrants& g, const LoadKnobs& k) {
  const int F = o.F, D = o.D, n = o.n, NB = o.NB, nk = o.nk, npanel = e.npanel;
  const std::vector<int32_t>& panel_jmax = e.panel_jmax;
  CholPlan c;
  // k_cholesky_global stages each panel's rows in LDS when x and 16 rows of S fit
  // (SG_CHOL_GSTAGE=0: never, so tests reach the unstaged instance at any size)
  c.gstage = (size_t)std::max(n, 1) * 8 * (1 + kCholNb) <= g.global && k.chol_gstage;
  c.window = npanel <= kJendSh;   // band ends cached in LDS
  for (int pk = 0; pk < npanel; ++pk)
    if (panel_jmax[pk] - pk * kCholNb > kCholWS) c.window = false;
  // tiled band Cholesky: every tile row's band within kTB tiles, x and z' of the whole system in LDS
  c.tiles = n > 0 && nk == 0 && npanel <= kTileMaxNT && !k.chol_window;
  for (int pk = 0; pk < npanel; ++pk)
    if ((panel_jmax[pk] + kCholNb - 1) / kCholNb - pk > kTB) c.tiles = false;
  // free intrinsics (one 16-wide border tile): the frame band on k_chol_tiles, the border by k_chol_border
  // (SG_CHOL_BORDER=0: the arrowhead k_cholesky_global)
  c.border = false;
  if (nk > 0 && NB > 0 && n - 6 * NB <= kCholNb && !k.chol_window && k.chol_border) {
    const int32_t* panel_bend = panel_jmax.data() + npanel;   // (the tail: nk > 0)
    const int ntf = (6 * NB + kCholNb - 1) / kCholNb;
    c.border = ntf <= kTileMaxNT;
    for (int pk = 0; pk < ntf; ++pk)
      if ((panel_bend[pk] + kCholNb - 1) / kCholNb - pk > kTB) c.border = false;
    if (c.border) {
      c.tiles = true;
      // q_K tiles and the candidate operands in LDS where they fit (else global q_K / chol_candidates)
      c.border_flags = 0;
      for (int f : {1, 2, 3})   // the last that fits: both, else the candidate operands, else the q_K tiles
        if (border_lds_doubles(ntf, f, F, D, n) * sizeof(double) <= g.border &&
            (!(f & 2) || (F <= kCandMax && D <= kCandMax)))
          c.border_flags = f;
    }
  }
  // dissected band: a second workgroup factors the bottom nd tile rows (reversed) while the first factors
  // the top rows [0, m), both meeting at a separator of ns <= 7 tile rows (k_chol_tiles); worth it from about 12
  // tile rows.  The separator must hold every band of the top part: ns(m) = max_{K<m} tend[K] - m.  The chain is
  // priced in phases as max(m, nd + h) + ns, h = kHandoffPhases for the bottom's hand-off, and the cheapest m is
  // taken, the smaller separator on a tie (C2, whose rows are 6-7 tiles wide: m = 7, ns = 5, nd = 6 — 12 phases on
  // the top chain instead of 14; C5, 8 tiles: ns = 7, nd = 33 as before).
  // SG_CHOL_SEP=7: the fixed 7-row separator (tests).
  c.nd = 0;
  c.ns = kTB - 1;
  if (c.tiles && !c.border && npanel >= kSplitMinNT && k.chol_split) {
    const bool fixed7 = k.chol_sep7;
    double best = 1e30;
    int reach = 0;   // max_{K<m} tend[K]
    for (int m = 1; m < npanel; ++m) {
      reach = std::max(reach, std::min(npanel, (panel_jmax[m - 1] + kCholNb - 1) / kCholNb));
      const int ns = fixed7 ? kTB - 1 : reach - m;
      const int nd = npanel - m - ns;
      if (ns < 1 || ns > kTB - 1 || reach - m > ns || nd < 2) continue;
      const double cost = std::max((double)m, nd + kHandoffPhases) + ns;
      if (cost < best || (cost == best && ns < c.ns)) {   // ties: the smaller separator
        best = cost;
        c.nd = nd;
        c.ns = ns;
      }
    }
  }
  if (c.tiles) {
    // W tiles of the top and bottom halves, the bottom's z' (+ failure slot), the separator contribution
    // and its rhs, the tile-major band St (PlanStile), then the constants {0, 1}
    c.wg_size = (size_t)2 * npanel * kTB * 256 + 16 * (size_t)npanel + 49 * 256 + 7 * 16 + stile_doubles(npanel) + 2;
    c.tile_lds = (size_t)npanel * 32 * sizeof(double) + (size_t)(3 * npanel + 1) / 2 * sizeof(double);
    c.cand_lds = !c.border && F <= kCandMax && D <= kCandMax &&
                 c.tile_lds + cand_lds_bytes(F, D, n) <= 100 * 1024 &&
                 c.tile_lds + cand_lds_bytes(F, D, n) <= g.tiles;
    if (c.cand_lds) c.tile_lds += cand_lds_bytes(F, D, n);
    if (c.tile_lds > g.tiles) {   // beyond the LDS granted at construction: the one-workgroup kernels
      c.tiles = false;
      c.border = false;
      c.nd = 0;
    }
  }
  return c;
}

// Where k_S_reduce's band tiles go in St (ba_plan.h), and the band ends of the reversed matrix the bottom
// workgroup factors.  Meaningful for the tiled Cholesky without border (nk = 0: the frame tiles are all of S).
StilePlan PlanStile(const Envelope& e, const CholPlan& c) {
  StilePlan s;
  const int NT = e.npanel;
  s.dst.assign(2 * (size_t)std::max(e.nstile, 1), -1);
  s.tend_rev.assign(std::max(NT, 1), 0);
  if (!c.tiles || c.border) return s;
  const int top_end = c.nd > 0 ? NT - c.nd : NT;   // m + ns: rows and columns of the top workgroup
  for (int t = 0; t < e.nstile; ++t) {
    const int R = e.stile[t] >> 16, C = e.stile[t] & 0xffff;
    if (C - R >= kTB || C >= NT) continue;
    if (C < top_end) {
      s.dst[2 * t] = R * kTB + (C - R);
    } else if (NT - 1 - R < c.nd + c.ns) {   // (a band tile of a column >= m + ns starts at a separator row or below)
      const int Ir = NT - 1 - C;
      s.dst[2 * t + 1] = NT * kTB + Ir * kTB + (C - R);
    }
  }
  std::vector<int> tend(NT);
  for (int R = 0; R < NT; ++R) tend[R] = std::min(NT, (e.panel_jmax[R] + kCholNb - 1) / kCholNb);
  for (int k = 0; k < NT; ++k) {
    const int col = NT - 1 - k;
    int lo = col;
    for (int R = col - 1; R >= 0; --R)
      if (tend[R] > col) lo = R;
    s.tend_rev[k] = NT - lo;
  }
  return s;
}

}  // namespace sg
