// ba_relpose.hip — relative pose of frame pairs from their shared observations: sg_slam_relative_poses.
//
// 8-point RANSAC with a fixed number of hypotheses (relpose_math.h: sampler, normalised 8-point, Sampson score,
// decomposition), all pairs of a call in two launches.
//
// k_relpose_ransac: n x S workgroups of 256 threads, S = H / 256, one thread per hypothesis.  The prologue undistorts
// the pair's first kRelStage records into LDS, four arrays (32 KiB); records beyond are read from global memory and
// undistorted at the read.  A thread draws its eight records, forms E, and scores it in one loop over all the pair's
// records in index order, every lane reading the same record (an LDS broadcast, or one global line).  The wave's best
// in loc_before's order comes from a shuffle butterfly, the four waves meet in LDS in wave order, and one candidate
// per workgroup is written.  Nothing passes between workgroups.
//
// k_relpose_select: one workgroup per pair.  The best of the pair's S candidates in slice order; its figures by a
// fixed-order reduction (thread t sums records t, t + 256, ... in index order, then the wave and workgroup sums: the
// reported costs are these, and can differ in the last bits from the index-order sum the candidates were ranked by); up to two rounds of local optimisation (normalisation sums, then the 45 moments of all
// inliers, each by a fixed-order workgroup reduction whose totals every thread holds, so every thread runs the same
// EssentialFromMoments and no result is handed round; then all records re-scored); the four decompositions' in-front
// and parallax counts in one pass; the status; the pose.  fp64 throughout, plain vector stores, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "ba_device.h"
#include "ba_pose.h"
#include "ba_relpose.h"
#include "relpose_math.h"

namespace sg {

namespace {

static_assert(kRelThreads == kPoseThreads, "the workgroup shape of the localization kernels");

struct RelRansacArgs {
  const RelPair* pairs;
  const int32_t* off;
  const double* records;   // 4 doubles per record: pixel in a, pixel in b
  RelCandidate* cand;      // [n * S]
  double tau2;
  uint32_t seed;
  int32_t S;
};

// Record i of the pair in plane coordinates, straight from global memory.
__device__ __forceinline__ void rel_global(const double* R, const double* ka, const double* kb, int i, double* xa,
                                           double* xb) {
  const double* r = R + 4 * (size_t)i;
  UndistortPixel(ka, r, xa);
  UndistortPixel(kb, r + 2, xb);
}

__global__ __launch_bounds__(kRelThreads) void k_relpose_ransac(RelRansacArgs a) {
  __shared__ double rec[4][kRelStage];
  __shared__ RelCandidate wbest[kRelThreads / 64];
  const int tid = threadIdx.x;
  const int pi = blockIdx.x / a.S, slice = blockIdx.x % a.S;
  const RelPair& pr = a.pairs[pi];
  if (!pr.run) return;   // (the whole workgroup: fewer than kRelMinObs records, decided by the planner)
  const int o0 = a.off[pi], cnt = a.off[pi + 1] - o0;
  const double* R = a.records + 4 * (size_t)o0;
  double ka[7], kb[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    ka[i] = pr.ka[i];
    kb[i] = pr.kb[i];
  }
  for (int i = tid; i < cnt && i < kRelStage; i += kRelThreads) {
    double xa[2], xb[2];
    rel_global(R, ka, kb, i, xa, xb);
    rec[0][i] = xa[0];
    rec[1][i] = xa[1];
    rec[2][i] = xb[0];
    rec[3][i] = xb[1];
  }
  __syncthreads();
  const double ifa[2] = {1.0 / ka[3], 1.0 / ka[4]}, ifb[2] = {1.0 / kb[3], 1.0 / kb[4]};

  const int h = slice * kRelThreads + tid;
  int32_t idx[kRelSample];
  RelSample(a.seed, (uint32_t)pr.a * 65536u + (uint32_t)pr.b, h, cnt, idx);
  double sa[kRelSample][2], sb[kRelSample][2];
#pragma unroll
  for (int j = 0; j < kRelSample; ++j) {
    const int i = idx[j];
    if (i < kRelStage) {
      sa[j][0] = rec[0][i];
      sa[j][1] = rec[1][i];
      sb[j][0] = rec[2][i];
      sb[j][1] = rec[3][i];
    } else {
      rel_global(R, ka, kb, i, sa[j], sb[j]);
    }
  }
  double E[9];
  const bool valid = RelEightPoint(sa, sb, E, nullptr);
  double ssum = 0.0;
  int inl = 0;
  if (valid) {
    const int staged = cnt < kRelStage ? cnt : kRelStage;
    for (int i = 0; i < staged; ++i) {   // every lane reads record i
      const double xa[2] = {rec[0][i], rec[1][i]}, xb[2] = {rec[2][i], rec[3][i]};
      const double e2 = RelSampson(E, xa, xb, ifa, ifb);
      const bool in = e2 <= a.tau2;   // (false for NaN)
      ssum += in ? e2 : 0.0;
      inl += in;
    }
    for (int i = staged; i < cnt; ++i) {
      double xa[2], xb[2];
      rel_global(R, ka, kb, i, xa, xb);
      const double e2 = RelSampson(E, xa, xb, ifa, ifb);
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
    RelCandidate c;
    c.cost = best.cost;
    c.sumsq = best.s;
#pragma unroll
    for (int i = 0; i < 9; ++i) c.E[i] = valid ? E[i] : 0.0;
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
    for (int i = 1; i < kRelThreads / 64; ++i) {
      total += wbest[i].models;
      const LocKey ki{wbest[i].cost, wbest[i].sumsq, wbest[i].inliers, wbest[i].h, 0};
      const LocKey kb2{wbest[bw].cost, wbest[bw].sumsq, wbest[bw].inliers, wbest[bw].h, 0};
      if (loc_before(ki, kb2)) bw = i;
    }
    RelCandidate c = wbest[bw];
    c.models = total;
    a.cand[blockIdx.x] = c;
  }
}

struct RelSelectArgs {
  const RelPair* pairs;
  const int32_t* off;
  const double* records;
  const RelCandidate* cand;   // [n * S]
  RelOut* out;                // [n]
  int32_t* flags;             // [off[n]] per-record inlier flags at the reported E
  double tau2, min_parallax;
  uint32_t seed;
  int32_t S, min_inliers, refine;
};

// The MSAC figures of E over all records: v[0] the inliers' e^2, v[1] their count; every thread gets the totals.
__device__ __forceinline__ void rel_score_all(const double* E, const double* R, const double* ka, const double* kb,
                                              const double* ifa, const double* ifb, int cnt, double tau2, double* red,
                                              double (&v)[2]) {
  v[0] = v[1] = 0.0;
  for (int i = threadIdx.x; i < cnt; i += kRelThreads) {
    double xa[2], xb[2];
    rel_global(R, ka, kb, i, xa, xb);
    const double e2 = RelSampson(E, xa, xb, ifa, ifb);
    const bool in = e2 <= tau2;
    v[0] += in ? e2 : 0.0;
    v[1] += in ? 1.0 : 0.0;
  }
  block_sum_multi<kRelThreads, 2>(v, red);
  __syncthreads();   // (red is reused by the next reduction)
}

__global__ __launch_bounds__(kRelThreads) void k_relpose_select(RelSelectArgs a) {
  __shared__ double sE[9];
  __shared__ double red[kRelMoments * (kRelThreads / 64)];
  __shared__ int pick[2];   // h | models
  const int tid = threadIdx.x;
  const int pi = blockIdx.x;
  const RelPair& pr = a.pairs[pi];
  if (!pr.run) return;   // (the whole workgroup) SG_REL_DID_NOT_RUN, reported by the host
  const int o0 = a.off[pi], cnt = a.off[pi + 1] - o0;
  const double* R = a.records + 4 * (size_t)o0;
  if (tid == 0) {
    const RelCandidate* C = a.cand + (size_t)pi * a.S;
    int best = 0, total = C[0].models;
    for (int s = 1; s < a.S; ++s) {
      total += C[s].models;
      const LocKey ks{C[s].cost, C[s].sumsq, C[s].inliers, C[s].h, 0};
      const LocKey kb2{C[best].cost, C[best].sumsq, C[best].inliers, C[best].h, 0};
      if (loc_before(ks, kb2)) best = s;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) sE[i] = C[best].E[i];
    pick[0] = C[best].h;
    pick[1] = total;
  }
  __syncthreads();
  const int bh = pick[0];
  if (bh < 0) {   // (the whole workgroup) no hypothesis gave a model
    if (tid == 0) {
      RelOut o{};
      o.status = SG_REL_NO_MODEL;
      o.num_obs = cnt;
      o.h = -1;
#pragma unroll
      for (int i = 0; i < 8; ++i) o.sample[i] = -1;
      a.out[pi] = o;
    }
    return;
  }
  double ka[7], kb[7], E[9];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    ka[i] = pr.ka[i];
    kb[i] = pr.kb[i];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) E[i] = sE[i];
  const double ifa[2] = {1.0 / ka[3], 1.0 / ka[4]}, ifb[2] = {1.0 / kb[3], 1.0 / kb[4]};
  double v[2];
  rel_score_all(E, R, ka, kb, ifa, ifb, cnt, a.tau2, red, v);
  LocKey cur{(double)(cnt - (int)v[1]) * a.tau2 + v[0], v[0], (int)v[1], bh, 0};
  const double ransac_cost = cur.cost;

  // local optimisation: every thread holds the same totals and runs the same arithmetic
  int refined = 0;
  for (int round = 0; round < 2 && a.refine && cur.inl >= kRelMinObs; ++round) {
    double st[7] = {0, 0, 0, 0, 0, 0, 0};   // count | a: sum x, sum y, sum x^2 + y^2 | b: the same
    for (int i = tid; i < cnt; i += kRelThreads) {
      double xa[2], xb[2];
      rel_global(R, ka, kb, i, xa, xb);
      if (RelSampson(E, xa, xb, ifa, ifb) <= a.tau2) {
        st[0] += 1.0;
        st[1] += xa[0]; st[2] += xa[1]; st[3] += xa[0] * xa[0] + xa[1] * xa[1];
        st[4] += xb[0]; st[5] += xb[1]; st[6] += xb[0] * xb[0] + xb[1] * xb[1];
      }
    }
    block_sum_multi<kRelThreads, 7>(st, red);
    __syncthreads();
    const double sta[4] = {st[0], st[1], st[2], st[3]}, stb[4] = {st[0], st[4], st[5], st[6]};
    double na[3], nb[3];
    if (!RelNormFrom(sta, na) || !RelNormFrom(stb, nb)) break;   // (uniform over the workgroup)
    double M[kRelMoments];
#pragma unroll
    for (int i = 0; i < kRelMoments; ++i) M[i] = 0.0;
    for (int i = tid; i < cnt; i += kRelThreads) {
      double xa[2], xb[2], row[9];
      rel_global(R, ka, kb, i, xa, xb);
      if (RelSampson(E, xa, xb, ifa, ifb) <= a.tau2) {
        RelRow(na, nb, xa, xb, row);
        RelMomentsAdd(row, M);
      }
    }
    block_sum_multi<kRelThreads, kRelMoments>(M, red);
    __syncthreads();
    double En[9];
    if (!EssentialFromMoments(M, na, nb, En, nullptr)) break;   // (uniform)
    rel_score_all(En, R, ka, kb, ifa, ifb, cnt, a.tau2, red, v);
    const LocKey nk{(double)(cnt - (int)v[1]) * a.tau2 + v[0], v[0], (int)v[1], bh, 0};
    if (loc_before(cur, nk)) break;   // after the current one: not kept, and a second round would repeat it
    cur = nk;
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = En[i];
    ++refined;
  }

  // the four decompositions on the inliers, and the inlier flags at the reported E
  double Rm[2][9], t[3];
  const bool dec = RelDecompose(E, Rm[0], Rm[1], t);   // (uniform)
  double c8[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // in front, per decomposition | in front with the parallax
  for (int i = tid; i < cnt; i += kRelThreads) {
    double xa[2], xb[2];
    rel_global(R, ka, kb, i, xa, xb);
    const bool in = RelSampson(E, xa, xb, ifa, ifb) <= a.tau2;
    a.flags[o0 + i] = in;
    if (!in || !dec) continue;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const double td[3] = {d & 1 ? -t[0] : t[0], d & 1 ? -t[1] : t[1], d & 1 ? -t[2] : t[2]};
      double da, db, g[3];
      if (RelDepths(Rm[d >> 1], td, xa, xb, &da, &db, g) && da > 0.0 && db > 0.0) {
        c8[d] += 1.0;
        if (RelParallax(g, xb) >= a.min_parallax) c8[4 + d] += 1.0;
      }
    }
  }
  block_sum_multi<kRelThreads, 8>(c8, red);
  if (tid == 0) {
    const int bd = RelVote(c8);   // (ties keep the earlier)
    RelOut o{};
    o.cost = cur.cost;
    o.sumsq = cur.s;
    o.ransac_cost = ransac_cost;
    o.num_obs = cnt;
    o.inliers = cur.inl;
    o.front = (int32_t)c8[bd];
    o.parallax = (int32_t)c8[4 + bd];
    o.refined = refined;
    o.h = bh;
    o.models = pick[1];
    RelSample(a.seed, (uint32_t)pr.a * 65536u + (uint32_t)pr.b, bh, cnt, o.sample);
    o.status = RelStatus(o.inliers, o.front, o.parallax, dec, a.min_inliers, a.min_parallax);
    // [t]x R of the four decompositions is -E, +E, +E, -E
    const double sign = (bd == 0 || bd == 3) ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.E[i] = dec ? sign * E[i] : E[i];
    if (dec) {
      const double td[3] = {bd & 1 ? -t[0] : t[0], bd & 1 ? -t[1] : t[1], bd & 1 ? -t[2] : t[2]};
      RelPoseOut(Rm[bd >> 1], td, o.q, o.t);
    }
    a.out[pi] = o;
  }
}

// q = q1 (x) q2 on Eigen memory [x, y, z, w]: the rotation of q1 after that of q2.
void QuatMul(const double* p, const double* q, double* r) {
  r[0] = p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1];
  r[1] = p[3] * q[1] - p[0] * q[2] + p[1] * q[3] + p[2] * q[0];
  r[2] = p[3] * q[2] + p[0] * q[1] - p[1] * q[0] + p[2] * q[3];
  r[3] = p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2];
}

}  // namespace

void RelPoseSolver::Solve(sg_map* m, const RelPlan& plan, int32_t n, const sg_relpose_options& o, int32_t* solved,
                          sg_relpose_result* results, int32_t* rec_offset, int32_t* rec_inlier, int32_t* rec_obs) {
  SG_REQUIRE(m && solved && n > 0 && (int32_t)plan.pairs.size() == n, SG_EINVAL, "bad argument");
  const int H = plan.H, S = plan.S;
  const size_t total = (size_t)plan.off[n];
  std::vector<sg_relpose_result> res((size_t)n, sg_relpose_result{});
  for (int i = 0; i < n; ++i) {
    res[i].status = SG_REL_DID_NOT_RUN;
    res[i].num_obs = plan.off[i + 1] - plan.off[i];
    res[i].hypotheses = H;
    res[i].best_hypothesis = -1;
    for (int j = 0; j < 8; ++j) res[i].best_sample[j] = -1;
  }
  timer_.Reset();
  if (plan.num_run > 0) {
    stream_.Bind();
    io_.Begin();
    io_.Up(pairs_, plan.pairs);
    io_.Up(off_, plan.off);
    io_.Up(records_, plan.records);
    cand_.Resize((size_t)n * S);
    out_.Resize((size_t)n);
    flags_.Resize(std::max<size_t>(total, 1));
    io_.FlushUp(stream_.get());
    RelRansacArgs ra{};
    ra.pairs = pairs_.ptr;
    ra.off = off_.ptr;
    ra.records = records_.ptr;
    ra.cand = cand_.ptr;
    ra.tau2 = o.threshold_px * o.threshold_px;
    ra.seed = o.seed;
    ra.S = S;
    RelSelectArgs sa{};
    sa.pairs = pairs_.ptr;
    sa.off = off_.ptr;
    sa.records = records_.ptr;
    sa.cand = cand_.ptr;
    sa.out = out_.ptr;
    sa.flags = flags_.ptr;
    sa.tau2 = ra.tau2;
    sa.min_parallax = o.min_parallax;
    sa.seed = o.seed;
    sa.S = S;
    sa.min_inliers = o.min_inliers;
    sa.refine = o.refine != 0;
    timer_.Start(stream_.get());
    hipLaunchKernelGGL(k_relpose_ransac, dim3((unsigned)plan.grid), dim3(kRelThreads), 0, stream_.get(), ra);
    SG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_relpose_select, dim3((unsigned)n), dim3(kRelThreads), 0, stream_.get(), sa);
    SG_HIP_CHECK(hipGetLastError());
    timer_.Stop(stream_.get());
    out_h_.resize((size_t)n);
    flags_h_.resize(total);
    io_.Down(out_h_.data(), out_.ptr, (size_t)n * sizeof(RelOut));
    io_.Down(flags_h_.data(), flags_.ptr, total * sizeof(int32_t));
    io_.FinishDown(stream_.get());
    timer_.Read();
    for (int i = 0; i < n; ++i) {
      if (!plan.pairs[i].run) continue;   // (its result was not written)
      const RelOut& w = out_h_[i];
      SG_REQUIRE(w.status >= SG_REL_OK && w.status <= SG_REL_LOW_PARALLAX && w.status != SG_REL_DID_NOT_RUN, SG_EDEVICE,
                 "relative-pose status out of range");
      SG_REQUIRE(w.num_obs == res[i].num_obs, SG_EDEVICE, "relative-pose result of another pair");
      sg_relpose_result& r = res[i];
      r.status = w.status;
      r.models = w.models;
      if (w.status == SG_REL_NO_MODEL) continue;
      SG_REQUIRE(w.h >= 0 && w.h < H && w.inliers >= 0 && w.inliers <= w.num_obs && w.front <= w.inliers &&
                     w.parallax <= w.front,
                 SG_EDEVICE, "relative-pose winner out of range");
      r.num_inliers = w.inliers;
      r.num_front = w.front;
      r.num_parallax = w.parallax;
      r.refined = w.refined;
      r.best_hypothesis = w.h;
      std::memcpy(r.best_sample, w.sample, sizeof(r.best_sample));
      r.msac_cost = w.cost;
      r.ransac_cost = w.ransac_cost;
      r.inlier_rms_px = w.inliers > 0 ? std::sqrt(w.sumsq / w.inliers) : 0.0;
      std::memcpy(r.q, w.q, sizeof(r.q));
      std::memcpy(r.t, w.t, sizeof(r.t));
      std::memcpy(r.E, w.E, sizeof(r.E));
    }
  }
  // write-back only after every pair's result has been checked: a failing call changes nothing.  Frame a's pose is
  // taken as it was at entry, also where a is the b of an earlier pair of the list.
  std::vector<double> qa((size_t)4 * n), ta((size_t)3 * n);
  for (int i = 0; i < n; ++i) {
    std::memcpy(&qa[4 * (size_t)i], m->q + 4 * (size_t)plan.pairs[i].a, 4 * sizeof(double));
    std::memcpy(&ta[3 * (size_t)i], m->t + 3 * (size_t)plan.pairs[i].a, 3 * sizeof(double));
  }
  for (int i = 0; i < n; ++i) {
    solved[i] = res[i].status == SG_REL_OK;
    if (rec_inlier)
      for (int32_t r = plan.off[i]; r < plan.off[i + 1]; ++r) rec_inlier[r] = solved[i] ? flags_h_[r] : -1;
    if (!solved[i] || !(o.baseline > 0.0)) continue;
    const double* q0 = &qa[4 * (size_t)i];
    const double* t0 = &ta[3 * (size_t)i];
    double q[4];
    QuatMul(res[i].q, q0, q);
    double inv = 1.0 / std::sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    if (q[3] < 0.0) inv = -inv;
    // R_a^T t_rel: the conjugate of q_a applied to t_rel (CameraPoint with a zero centre)
    const double qc[4] = {-q0[0], -q0[1], -q0[2], q0[3]}, zero[3] = {0, 0, 0};
    const double X[4] = {res[i].t[0], res[i].t[1], res[i].t[2], 1.0};
    double vv[3], w[3];
    CameraPoint(qc, zero, X, vv, w);
    double* qb = m->q + 4 * (size_t)plan.pairs[i].b;
    double* tb = m->t + 3 * (size_t)plan.pairs[i].b;
    for (int c = 0; c < 4; ++c) qb[c] = q[c] * inv;
    for (int c = 0; c < 3; ++c) tb[c] = t0[c] + o.baseline * w[c];
  }
  if (rec_offset) std::memcpy(rec_offset, plan.off.data(), ((size_t)n + 1) * sizeof(int32_t));
  if (rec_obs && total) std::memcpy(rec_obs, plan.obs.data(), 2 * total * sizeof(int32_t));
  if (results)
    for (int i = 0; i < n; ++i) results[i] = res[i];
}

}  // namespace sg
