// ba_align.hip — alignment of matched landmarks by a similarity transform: sg_slam_align_points.
//
// 3-point Sim(3) RANSAC with a fixed number of hypotheses (pnp_math.h: the sampler; align_math.h: Horn's closed form
// and the residual), all groups of a call in two launches.  The 3D-3D sibling of k_pose_ransac / k_pose_select.
//
// k_align_ransac: n x S workgroups of 256 threads, S = H / 256, one thread per hypothesis.  The prologue stages the
// group's first kAlignStage records into LDS, six arrays (48 KiB); records beyond are read from global memory.  A
// thread draws its three records, runs Horn (the 4x4 Jacobi in registers), and scores the transform in one loop over
// all the group's records in index order, every lane reading the same record (an LDS broadcast, or one global line),
// with no barrier and no reduction inside.  The wave's best in loc_before's order comes from a shuffle butterfly, the
// four waves meet in LDS in wave order, and one candidate per workgroup is written.  Nothing passes between
// workgroups.
//
// k_align_select: one workgroup per group.  The best of the group's S candidates in slice order; its figures by a
// fixed-order reduction (thread t sums records t, t + 256, ... in index order, then the wave and workgroup sums: the
// reported costs are these, and can differ in the last bits from the index-order sum the candidates were ranked by);
// then, in a loop, the current inliers' flags, centroids and centred moments (two fixed-order reductions), Horn on
// them in thread 0, handed round through LDS; that gives the gap of the current inliers and the next transform of the
// local optimisation, which is re-scored on all records and kept when its key is not after the current one (at most
// two rounds).  The loop always ends on a moment pass over the reported transform's inliers, so the flags and the gap
// are the final ones, with refine == 0 too.  fp64 throughout, plain vector stores, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "align_math.h"
#include "ba_align.h"
#include "ba_device.h"
#include "ba_pose.h"
#include "pnp_math.h"

namespace sg {

namespace {

static_assert(kAlignThreads == kPoseThreads, "the workgroup shape of the localization kernels");
static_assert(kAlignMaxHypotheses == kLocalizeMaxHypotheses, "capped as in localize");

struct AlignRansacArgs {
  const AlignGroup* groups;
  const int32_t* off;
  const double* records;   // 6 doubles per record: X_a then X_b, Euclidean
  AlignCandidate* cand;    // [n * S]
  double tau2, max_scale;
  uint32_t seed;
  int32_t S, fix_scale;
};

__global__ __launch_bounds__(kAlignThreads) void k_align_ransac(AlignRansacArgs a) {
  __shared__ double rec[6][kAlignStage];
  __shared__ AlignCandidate wbest[kAlignThreads / 64];
  const int tid = threadIdx.x;
  const int gi = blockIdx.x / a.S, slice = blockIdx.x % a.S;
  const AlignGroup gr = a.groups[gi];
  if (!gr.run) return;   // (the whole workgroup: fewer than kAlignMinRecords records, decided by the planner)
  const int o0 = a.off[gi], cnt = a.off[gi + 1] - o0;
  const double* R = a.records + 6 * (size_t)o0;
  const int staged = cnt < kAlignStage ? cnt : kAlignStage;
  for (int i = tid; i < staged; i += kAlignThreads) {
#pragma unroll
    for (int c = 0; c < 6; ++c) rec[c][i] = R[6 * (size_t)i + c];
  }
  __syncthreads();

  const int h = slice * kAlignThreads + tid;
  int32_t idx[3];
  PnpSample(a.seed, gr.key, h, cnt, idx);
  double smp[18];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int i = idx[j];
#pragma unroll
    for (int c = 0; c < 6; ++c) smp[6 * j + c] = i < kAlignStage ? rec[c][i] : R[6 * (size_t)i + c];
  }
  AlignXf xf;
  double gap;
  const bool valid = AlignHorn(smp, 3, a.fix_scale, a.max_scale, &xf, &gap);
  double ssum = 0.0;
  int inl = 0;
  if (valid) {
    double A[9];
    AlignMatrix(xf.s, xf.q, A);
    for (int i = 0; i < staged; ++i) {   // every lane reads record i
      const double X[3] = {rec[0][i], rec[1][i], rec[2][i]}, Y[3] = {rec[3][i], rec[4][i], rec[5][i]};
      const double e2 = AlignResidual2(A, xf.t, X, Y);
      const bool in = e2 <= a.tau2;   // (false for NaN)
      ssum += in ? e2 : 0.0;
      inl += in;
    }
    for (int i = staged; i < cnt; ++i) {
      const double* r = R + 6 * (size_t)i;
      const double e2 = AlignResidual2(A, xf.t, r, r + 3);
      const bool in = e2 <= a.tau2;
      ssum += in ? e2 : 0.0;
      inl += in;
    }
  }
  LocKey best{0.0, 0.0, 0, -1, 0};
  if (valid) best = LocKey{(double)(cnt - inl) * a.tau2 + ssum, ssum, inl, h, 0};

  // the wave's best: butterfly on the key; the order is total, so every lane ends with the same key
  LocKey w = best;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    LocKey o;
    o.cost = __shfl_xor(w.cost, d);
    o.s = __shfl_xor(w.s, d);
    o.inl = __shfl_xor(w.inl, d);
    o.h = __shfl_xor(w.h, d);
    o.root = 0;
    if (loc_before(o, w)) w = o;
  }
  const int models = __popcll(__ballot(valid));
  const int wave = tid >> 6;
  if (w.h >= 0 ? w.h == h : (tid & 63) == 0) {   // the winning lane, or lane 0 of a wave without a model
    AlignCandidate c;
    c.cost = best.cost;
    c.sumsq = best.s;
    c.s = valid ? xf.s : 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) c.q[i] = valid ? xf.q[i] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) c.t[i] = valid ? xf.t[i] : 0.0;
    c.h = best.h;
    c.inliers = best.inl;
    c.models = models;
    c.pad = 0;
    wbest[wave] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int bw = 0, total = wbest[0].models;
#pragma unroll
    for (int i = 1; i < kAlignThreads / 64; ++i) {
      total += wbest[i].models;
      const LocKey ki{wbest[i].cost, wbest[i].sumsq, wbest[i].inliers, wbest[i].h, 0};
      const LocKey kb{wbest[bw].cost, wbest[bw].sumsq, wbest[bw].inliers, wbest[bw].h, 0};
      if (loc_before(ki, kb)) bw = i;
    }
    AlignCandidate c = wbest[bw];
    c.models = total;
    a.cand[blockIdx.x] = c;
  }
}

struct AlignSelectArgs {
  const AlignGroup* groups;
  const int32_t* off;
  const double* records;
  const AlignCandidate* cand;   // [n * S]
  AlignOut* out;                // [n]
  int32_t* flags;               // [off[n]] per-record inlier flags at the reported transform
  double tau2, max_scale, min_gap;
  uint32_t seed;
  int32_t S, min_inliers, refine, fix_scale;
};

// The MSAC figures of a transform over all records: v[0] the inliers' e^2, v[1] their count; every thread gets the
// totals.
__device__ __forceinline__ void align_score_all(const double* A, const double* t, const double* R, int cnt, double tau2,
                                                double* red, double (&v)[2]) {
  v[0] = v[1] = 0.0;
  for (int i = threadIdx.x; i < cnt; i += kAlignThreads) {
    const double* r = R + 6 * (size_t)i;
    const double e2 = AlignResidual2(A, t, r, r + 3);
    const bool in = e2 <= tau2;
    v[0] += in ? e2 : 0.0;
    v[1] += in ? 1.0 : 0.0;
  }
  block_sum_multi<kAlignThreads, 2>(v, red);
  __syncthreads();   // (red is reused by the next reduction)
}

__global__ __launch_bounds__(kAlignThreads) void k_align_select(AlignSelectArgs a) {
  __shared__ double sX[8];    // the picked candidate: s, q, t
  __shared__ double sH[10];   // Horn on the current inliers: s, q, t, 1 when it gave a model, the gap
  __shared__ double red[kAlignMoments * (kAlignThreads / 64)];
  __shared__ int pick[2];     // h | models
  const int tid = threadIdx.x;
  const int gi = blockIdx.x;
  const AlignGroup gr = a.groups[gi];
  if (!gr.run) return;   // (the whole workgroup) SG_ALIGN_DID_NOT_RUN, reported by the host
  const int o0 = a.off[gi], cnt = a.off[gi + 1] - o0;
  const double* R = a.records + 6 * (size_t)o0;
  if (tid == 0) {
    const AlignCandidate* C = a.cand + (size_t)gi * a.S;
    int best = 0, total = C[0].models;
    for (int s = 1; s < a.S; ++s) {
      total += C[s].models;
      const LocKey ks{C[s].cost, C[s].sumsq, C[s].inliers, C[s].h, 0};
      const LocKey kb{C[best].cost, C[best].sumsq, C[best].inliers, C[best].h, 0};
      if (loc_before(ks, kb)) best = s;
    }
    sX[0] = C[best].s;
#pragma unroll
    for (int i = 0; i < 4; ++i) sX[1 + i] = C[best].q[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) sX[5 + i] = C[best].t[i];
    pick[0] = C[best].h;
    pick[1] = total;
  }
  __syncthreads();
  const int bh = pick[0];
  if (bh < 0) {   // (the whole workgroup) no hypothesis gave a model
    if (tid == 0) {
      AlignOut o{};
      o.status = SG_ALIGN_NO_MODEL;
      o.num_records = cnt;
      o.h = -1;
#pragma unroll
      for (int i = 0; i < 3; ++i) o.sample[i] = -1;
      a.out[gi] = o;
    }
    return;
  }
  AlignXf xf;
  xf.s = sX[0];
#pragma unroll
  for (int i = 0; i < 4; ++i) xf.q[i] = sX[1 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) xf.t[i] = sX[5 + i];
  double A[9];
  AlignMatrix(xf.s, xf.q, A);
  double v[2];
  align_score_all(A, xf.t, R, cnt, a.tau2, red, v);
  LocKey cur{(double)(cnt - (int)v[1]) * a.tau2 + v[0], v[0], (int)v[1], bh, 0};
  const double ransac_cost = cur.cost;

  int refined = 0;
  double gap = 0.0;
  for (int round = 0;; ++round) {   // (every branch below is uniform over the workgroup)
    // the current inliers: their flags, count and coordinate sums
    double st[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < cnt; i += kAlignThreads) {
      const double* r = R + 6 * (size_t)i;
      const bool in = AlignResidual2(A, xf.t, r, r + 3) <= a.tau2;
      a.flags[o0 + i] = in;
      if (in) {
        st[0] += 1.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) st[1 + c] += r[c];
      }
    }
    block_sum_multi<kAlignThreads, 7>(st, red);
    __syncthreads();
    const double inv = st[0] > 0.0 ? 1.0 / st[0] : 0.0;
    const double xm[3] = {st[1] * inv, st[2] * inv, st[3] * inv}, ym[3] = {st[4] * inv, st[5] * inv, st[6] * inv};
    double M[kAlignMoments];
#pragma unroll
    for (int i = 0; i < kAlignMoments; ++i) M[i] = 0.0;
    for (int i = tid; i < cnt; i += kAlignThreads) {
      const double* r = R + 6 * (size_t)i;
      if (AlignResidual2(A, xf.t, r, r + 3) <= a.tau2) AlignMomentsAdd(r, r + 3, xm, ym, M);
    }
    block_sum_multi<kAlignThreads, kAlignMoments>(M, red);
    __syncthreads();
    if (tid == 0) {
      AlignXf nx{};
      double g = 0.0;
      const bool ok = st[0] > 0.0 && AlignFromMoments(xm, ym, M, a.fix_scale, a.max_scale, &nx, &g);
      sH[0] = nx.s;
#pragma unroll
      for (int i = 0; i < 4; ++i) sH[1 + i] = nx.q[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) sH[5 + i] = nx.t[i];
      sH[8] = ok ? 1.0 : 0.0;
      sH[9] = g;
    }
    __syncthreads();
    gap = sH[9];
    if (!a.refine || round == 2 || cur.inl < kAlignMinRecords || sH[8] == 0.0) break;
    AlignXf nx;
    nx.s = sH[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) nx.q[i] = sH[1 + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) nx.t[i] = sH[5 + i];
    double An[9];
    AlignMatrix(nx.s, nx.q, An);
    align_score_all(An, nx.t, R, cnt, a.tau2, red, v);   // (its barriers also fence sH before the next round's write)
    const LocKey nk{(double)(cnt - (int)v[1]) * a.tau2 + v[0], v[0], (int)v[1], bh, 0};
    if (loc_before(cur, nk)) break;   // after the current one: not kept, and a second round would repeat it
    cur = nk;
    xf = nx;
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = An[i];
    ++refined;
  }

  if (tid == 0) {
    AlignOut o{};
    o.cost = cur.cost;
    o.sumsq = cur.s;
    o.ransac_cost = ransac_cost;
    o.gap = gap;
    o.s = xf.s;
#pragma unroll
    for (int i = 0; i < 4; ++i) o.q[i] = xf.q[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = xf.t[i];
    o.status = AlignStatus(cur.inl, gap, a.min_inliers, a.min_gap);
    o.num_records = cnt;
    o.inliers = cur.inl;
    o.refined = refined;
    o.h = bh;
    o.models = pick[1];
    PnpSample(a.seed, gr.key, bh, cnt, o.sample);
    a.out[gi] = o;
  }
}

}  // namespace

void AlignSolver::Solve(const AlignPlan& plan, int32_t n, int32_t num_corr, const sg_align_options& o, int32_t* solved,
                        sg_align_result* results, int32_t* corr_inlier) {
  SG_REQUIRE(solved && n > 0 && num_corr >= 0 && (int32_t)plan.groups.size() == n, SG_EINVAL, "bad argument");
  const int H = plan.H, S = plan.S;
  const size_t total = (size_t)plan.off[n];
  std::vector<sg_align_result> res((size_t)n, sg_align_result{});
  for (int i = 0; i < n; ++i) {
    res[i].status = SG_ALIGN_DID_NOT_RUN;
    res[i].num_corr = plan.groups[i].num_corr;
    res[i].num_records = plan.off[i + 1] - plan.off[i];
    res[i].hypotheses = H;
    res[i].best_hypothesis = -1;
    for (int j = 0; j < 3; ++j) res[i].best_sample[j] = -1;
  }
  timer_.Reset();
  if (plan.num_run > 0) {
    stream_.Bind();
    io_.Begin();
    io_.Up(groups_, plan.groups);
    io_.Up(off_, plan.off);
    io_.Up(records_, plan.records);
    cand_.Resize((size_t)n * S);
    out_.Resize((size_t)n);
    flags_.Resize(std::max<size_t>(total, 1));
    io_.FlushUp(stream_.get());
    AlignRansacArgs ra{};
    ra.groups = groups_.ptr;
    ra.off = off_.ptr;
    ra.records = records_.ptr;
    ra.cand = cand_.ptr;
    ra.tau2 = o.threshold * o.threshold;
    ra.max_scale = o.max_scale;
    ra.seed = o.seed;
    ra.S = S;
    ra.fix_scale = o.fix_scale != 0;
    AlignSelectArgs sa{};
    sa.groups = groups_.ptr;
    sa.off = off_.ptr;
    sa.records = records_.ptr;
    sa.cand = cand_.ptr;
    sa.out = out_.ptr;
    sa.flags = flags_.ptr;
    sa.tau2 = ra.tau2;
    sa.max_scale = o.max_scale;
    sa.min_gap = o.min_gap;
    sa.seed = o.seed;
    sa.S = S;
    sa.min_inliers = o.min_inliers;
    sa.refine = o.refine != 0;
    sa.fix_scale = ra.fix_scale;
    timer_.Start(stream_.get());
    hipLaunchKernelGGL(k_align_ransac, dim3((unsigned)plan.grid), dim3(kAlignThreads), 0, stream_.get(), ra);
    SG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_align_select, dim3((unsigned)n), dim3(kAlignThreads), 0, stream_.get(), sa);
    SG_HIP_CHECK(hipGetLastError());
    timer_.Stop(stream_.get());
    out_h_.resize((size_t)n);
    flags_h_.resize(total);
    io_.Down(out_h_.data(), out_.ptr, (size_t)n * sizeof(AlignOut));
    io_.Down(flags_h_.data(), flags_.ptr, total * sizeof(int32_t));
    io_.FinishDown(stream_.get());
    timer_.Read();
    for (int i = 0; i < n; ++i) {
      if (!plan.groups[i].run) continue;   // (its result was not written)
      const AlignOut& w = out_h_[i];
      SG_REQUIRE(w.status >= SG_ALIGN_OK && w.status <= SG_ALIGN_DEGENERATE && w.status != SG_ALIGN_DID_NOT_RUN,
                 SG_EDEVICE, "alignment status out of range");
      SG_REQUIRE(w.num_records == res[i].num_records, SG_EDEVICE, "alignment result of another group");
      sg_align_result& r = res[i];
      r.status = w.status;
      r.models = w.models;
      if (w.status == SG_ALIGN_NO_MODEL) continue;
      SG_REQUIRE(w.h >= 0 && w.h < H && w.inliers >= 0 && w.inliers <= w.num_records && w.refined >= 0 &&
                     w.refined <= 2,
                 SG_EDEVICE, "alignment winner out of range");
      r.num_inliers = w.inliers;
      r.refined = w.refined;
      r.best_hypothesis = w.h;
      std::memcpy(r.best_sample, w.sample, sizeof(r.best_sample));
      r.msac_cost = w.cost;
      r.ransac_cost = w.ransac_cost;
      r.inlier_rms = w.inliers > 0 ? std::sqrt(w.sumsq / w.inliers) : 0.0;
      r.gap = w.gap;
      r.scale = w.s;
      std::memcpy(r.q, w.q, sizeof(r.q));
      std::memcpy(r.t, w.t, sizeof(r.t));
    }
  }
  // outputs only after every group's result has been checked: a failing call writes nothing
  for (int i = 0; i < n; ++i) solved[i] = res[i].status == SG_ALIGN_OK;
  if (corr_inlier) {
    for (int32_t j = 0; j < num_corr; ++j) corr_inlier[j] = -1;
    for (int i = 0; i < n; ++i) {
      if (!solved[i]) continue;
      for (int32_t r = plan.off[i]; r < plan.off[i + 1]; ++r) corr_inlier[plan.rec_corr[r]] = flags_h_[r];
    }
  }
  if (results)
    for (int i = 0; i < n; ++i) results[i] = res[i];
}

}  // namespace sg
