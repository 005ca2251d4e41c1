// ba_localize.hip — localization from scratch: sg_slam_localize_frames.
//
// Each listed frame's pose from its records alone (the pose at entry is not read): P3P RANSAC with a fixed number
// of hypotheses (pnp_math.h: sampler, Grunert's P3P, MSAC score), the status rules, and optionally k_pose_lm
// (ba_pose.hip) as the polish, started at the winner on the same stream.
//
// k_pose_ransac: n x S workgroups of 256 threads, S = H / 256, one thread per hypothesis.  The prologue stages the
// frame's first kPoseStage records into LDS in k_pose_lm's layout (six arrays, 48 KiB).  A thread draws its three
// records, solves the quartic, forms the pose of each root, and scores the poses side by side in one loop over all
// the frame's records, in index order, in which every lane reads the same record (an LDS broadcast, or one global
// line), with no reduction and no barrier inside.  The thread keeps its best root; the wave's best in loc_before's
// order comes from a shuffle butterfly (the order is total, so any butterfly gives the same winner), the four waves
// meet in LDS in wave order, and one candidate per workgroup is written.  Nothing passes between workgroups.
//
// k_pose_select: one workgroup per listed frame.  First launch: the best of the frame's S candidates in slice
// order, the winner's per-record inlier flags, and the inlier count and the inliers' sum of squares by a fixed-order
// reduction (the MSAC cost is (N - count) tau^2 + sum); the status; and the winner goes into the PoseFrame array
// k_pose_lm reads (q, t, run = status is OK), the way k_point_triangulate rewrites PointStart.  Second launch (after
// the polish): the same figures at PoseOut's pose.  The host applies the not-worse rule from the two sets of figures.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "ba_device.h"
#include "ba_pose.h"
#include "pnp_math.h"

namespace sg {

namespace {

struct RansacArgs {
  const PoseFrame* frames;
  const int32_t* off;
  const double* records;        // PoseRecord as 6 doubles
  const int32_t* frame_index;   // the listed frames' map indices (the sampler's key)
  LocCandidate* cand;           // [n * S]
  double tau2;
  uint32_t seed;
  int32_t S;
};

// Record i of the frame: from the LDS stage, or beyond it from global memory.
__device__ __forceinline__ void loc_record(const double (*rec)[kPoseStage], const double* R, int i, double* pt,
                                           double* X) {
  if (i < kPoseStage) {
    pt[0] = rec[0][i];
    pt[1] = rec[1][i];
#pragma unroll
    for (int a = 0; a < 4; ++a) X[a] = rec[2 + a][i];
  } else {
    const double* r = R + 6 * (size_t)i;
    pt[0] = r[0];
    pt[1] = r[1];
#pragma unroll
    for (int a = 0; a < 4; ++a) X[a] = r[2 + a];
  }
}

// (LocKey and loc_before, the order of the poses of one frame, are in ba_pose.h: k_relpose_* use them too.)
__device__ __forceinline__ LocKey loc_key(const LocCandidate& c) {
  return LocKey{c.cost, c.sumsq, c.inliers, c.h, c.root};
}

__global__ __launch_bounds__(kPoseThreads) void k_pose_ransac(RansacArgs a) {
  __shared__ double rec[6][kPoseStage];
  __shared__ double kk[7];
  __shared__ LocCandidate wbest[kPoseWaves];
  const int tid = threadIdx.x;
  const int fi = blockIdx.x / a.S, slice = blockIdx.x % a.S;
  const PoseFrame& fr = a.frames[fi];
  if (!fr.run) return;   // (the whole workgroup: fewer than kLocalizeMinObs records, decided by the planner)
  const int o0 = a.off[fi], cnt = a.off[fi + 1] - o0;
  const double* R = a.records + 6 * (size_t)o0;
  for (int i = tid; i < cnt && i < kPoseStage; i += kPoseThreads) {
    const double* r = R + 6 * (size_t)i;
#pragma unroll
    for (int j = 0; j < 6; ++j) rec[j][i] = r[j];
  }
  if (tid < 7) kk[tid] = fr.k[tid];
  __syncthreads();
  double k[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) k[i] = kk[i];

  const int h = slice * kPoseThreads + tid;
  int32_t idx[3];
  PnpSample(a.seed, a.frame_index[fi], h, cnt, idx);
  double f[3][3], P[3][3];
  bool usable = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double pt[2], X[4];
    loc_record(rec, R, idx[j], pt, X);
    if (!PnpEuclidean(X, P[j])) usable = false;
    PnpBearing(k, pt, f[j]);
  }
  P3pProblem pr;
  double v[4];
  int nroots = 0;
  if (usable && P3pSetup(f, P, &pr)) nroots = P3pQuartic(pr, v);

  // the roots' poses first, then one loop over the records that scores them side by side: the record is read once,
  // and the (up to four) independent chains of arithmetic hide each other's latency.  Every index below is a
  // compile-time constant after unrolling, so q, t and the sums stay in registers.
  double q[4][4], t[4][3], ssum[4];
  int inl[4];
  bool valid[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    valid[r] = r < nroots && P3pPose(f, P, pr, v[r], q[r], t[r]);
    ssum[r] = 0.0;
    inl[r] = 0;
  }
  if (valid[0] || valid[1] || valid[2] || valid[3]) {
    for (int i = 0; i < cnt; ++i) {   // every lane reads record i
      double pt[2], X[4];
      loc_record(rec, R, i, pt, X);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (!valid[r]) continue;
        int in;
        const double term = PnpScore(q[r], t[r], k, X, pt, a.tau2, &in);
        ssum[r] += in ? term : 0.0;   // (each root's sum runs in record order)
        inl[r] += in;
      }
    }
  }
  LocKey best{0.0, 0.0, 0, -1, -1};
  double bq[4] = {0, 0, 0, 1}, bt[3] = {0, 0, 0};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (!valid[r]) continue;
    const LocKey key{(double)(cnt - inl[r]) * a.tau2 + ssum[r], ssum[r], inl[r], h, r};
    if (loc_before(key, best)) {   // (a full tie keeps the smaller root index)
      best = key;
#pragma unroll
      for (int c = 0; c < 4; ++c) bq[c] = q[r][c];
#pragma unroll
      for (int c = 0; c < 3; ++c) bt[c] = t[r][c];
    }
  }

  // the wave's best: butterfly on the key; the order is total, so every lane ends with the same key
  LocKey w = best;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    LocKey o;
    o.cost = __shfl_xor(w.cost, d);
    o.s = __shfl_xor(w.s, d);
    o.inl = __shfl_xor(w.inl, d);
    o.h = __shfl_xor(w.h, d);
    o.root = __shfl_xor(w.root, d);
    if (loc_before(o, w)) w = o;
  }
  const int models = __popcll(__ballot(best.h >= 0));
  const int wave = tid >> 6;
  if (w.h >= 0 ? w.h == h : (tid & 63) == 0) {   // the winning lane, or lane 0 of a wave without a pose
    LocCandidate c;
    c.cost = best.cost;
    c.sumsq = best.s;
#pragma unroll
    for (int i = 0; i < 4; ++i) c.q[i] = bq[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) c.t[i] = bt[i];
    c.h = best.h;
    c.root = best.root;
    c.inliers = best.inl;
    c.models = models;
    wbest[wave] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int bw = 0, total = wbest[0].models;
#pragma unroll
    for (int i = 1; i < kPoseWaves; ++i) {
      total += wbest[i].models;
      if (loc_before(loc_key(wbest[i]), loc_key(wbest[bw]))) bw = i;
    }
    LocCandidate c = wbest[bw];
    c.models = total;
    a.cand[blockIdx.x] = c;
  }
}

struct SelectArgs {
  PoseFrame* frames;            // first launch: q, t, run rewritten for k_pose_lm
  const int32_t* off;
  const double* records;
  const int32_t* frame_index;
  const LocCandidate* cand;     // [n * S]
  const PoseOut* lm;            // second launch: the polish's poses
  LocOut* out;                  // [n]
  int32_t* flags;               // [off[n]] per-record inlier flags at the scored pose
  double tau2;
  uint32_t seed;
  int32_t S, min_inliers;
  int32_t post;                 // 0: first launch, 1: second
};

__global__ __launch_bounds__(kPoseThreads) void k_pose_select(SelectArgs a) {
  __shared__ double pose[8], kk[7];
  __shared__ double red[2 * kPoseWaves];
  __shared__ int pick[4];   // h | root | models
  const int tid = threadIdx.x;
  const int fi = blockIdx.x;
  PoseFrame& fr = a.frames[fi];
  if (!fr.run) return;   // (the whole workgroup) first launch: DID_NOT_RUN; second: not SG_LOC_OK, no polish
  const int o0 = a.off[fi], cnt = a.off[fi + 1] - o0;
  const double* R = a.records + 6 * (size_t)o0;
  if (tid == 0) {
    if (a.post) {
      const PoseOut& o = a.lm[fi];
#pragma unroll
      for (int i = 0; i < 4; ++i) pose[i] = o.q[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) pose[4 + i] = o.t[i];
      pick[0] = 0;
      pick[1] = 0;
      pick[2] = 0;
    } else {
      const LocCandidate* C = a.cand + (size_t)fi * a.S;
      int best = 0, total = C[0].models;
      for (int s = 1; s < a.S; ++s) {
        total += C[s].models;
        if (loc_before(loc_key(C[s]), loc_key(C[best]))) best = s;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) pose[i] = C[best].q[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) pose[4 + i] = C[best].t[i];
      pick[0] = C[best].h;
      pick[1] = C[best].root;
      pick[2] = total;
    }
  }
  if (tid < 7) kk[tid] = fr.k[tid];
  __syncthreads();
  const int bh = pick[0];
  if (bh < 0) {   // (the whole workgroup) no hypothesis gave a pose
    if (tid == 0) {
      LocOut o{};
      o.status = SG_LOC_NO_MODEL;
      o.num_obs = cnt;
      o.h = -1;
      o.root = -1;
      o.sample[0] = o.sample[1] = o.sample[2] = -1;
      o.models = 0;
      a.out[fi] = o;
      fr.run = 0;
    }
    return;
  }
  double q[4], t[3], k[7];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = pose[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = pose[4 + i];
#pragma unroll
  for (int i = 0; i < 7; ++i) k[i] = kk[i];
  double v[2] = {0.0, 0.0};   // the inliers' e^2 | their count (exact in a double)
  for (int i = tid; i < cnt; i += kPoseThreads) {
    const double* r = R + 6 * (size_t)i;
    int in;
    const double term = PnpScore(q, t, k, r + 2, r, a.tau2, &in);
    a.flags[o0 + i] = in;
    v[0] += in ? term : 0.0;
    v[1] += in;
  }
  block_sum_multi<kPoseThreads, 2>(v, red);   // (every thread of the block: all lanes active)
  if (tid == 0) {
    LocOut o{};
    o.sumsq = v[0];
    o.inliers = (int32_t)v[1];
    o.cost = (double)(cnt - o.inliers) * a.tau2 + o.sumsq;
    o.num_obs = cnt;
    const int need = a.min_inliers > kLocalizeMinObs ? a.min_inliers : kLocalizeMinObs;
    o.status = a.post || o.inliers >= need ? SG_LOC_OK : SG_LOC_FEW_INLIERS;
#pragma unroll
    for (int i = 0; i < 4; ++i) o.q[i] = q[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = t[i];
    o.h = bh;
    o.root = pick[1];
    o.models = pick[2];
    o.sample[0] = o.sample[1] = o.sample[2] = -1;
    if (!a.post) {
      PnpSample(a.seed, a.frame_index[fi], bh, cnt, o.sample);
#pragma unroll
      for (int i = 0; i < 4; ++i) fr.q[i] = q[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) fr.t[i] = t[i];
      fr.run = o.status == SG_LOC_OK;
    }
    a.out[fi] = o;
  }
}

}  // namespace

void PoseSolver::Localize(sg_map* m, const int32_t* frames, int32_t n, const sg_localize_options& lo,
                          const sg_solver_options& o, int32_t* solved, sg_localize_result* results,
                          int32_t* obs_inlier, sg_solver_summary* summaries) {
  SG_REQUIRE(m && (n == 0 || (frames && solved)), SG_EINVAL, "null argument");
  SG_REQUIRE(lo.threshold_px > 0.0, SG_EINVAL, "threshold_px must be positive");
  SG_REQUIRE(lo.max_hypotheses > 0, SG_EINVAL, "max_hypotheses must be positive");
  PlanPoses(*m, frames, n, false, &plan_, kLocalizeMinObs, true);
  const int H = (std::min(lo.max_hypotheses, kLocalizeMaxHypotheses) + kPoseThreads - 1) / kPoseThreads * kPoseThreads;
  const int S = H / kPoseThreads;
  const bool refine = lo.refine != 0;
  sg_solver_summary none{};
  none.termination_type = SG_DID_NOT_RUN;
  sums_.assign((size_t)n, none);
  std::vector<sg_localize_result> res((size_t)n, sg_localize_result{});
  std::vector<uint8_t> use_post((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    res[i].status = SG_LOC_DID_NOT_RUN;
    res[i].num_obs = plan_.off[i + 1] - plan_.off[i];
    res[i].hypotheses = H;
    res[i].best_hypothesis = -1;
    res[i].best_sample[0] = res[i].best_sample[1] = res[i].best_sample[2] = -1;
    // the pose at entry is not read: the slots k_pose_select fills for k_pose_lm go up as the identity
    PoseFrame& pf = plan_.frames[i];
    pf.q[0] = pf.q[1] = pf.q[2] = 0.0;
    pf.q[3] = 1.0;
    pf.t[0] = pf.t[1] = pf.t[2] = 0.0;
  }
  timer_.Reset();
  const size_t total = (size_t)plan_.off[n];
  if (plan_.num_run > 0) {
    stream_.Bind();
    io_.Begin();
    io_.Up(frames_, plan_.frames);
    io_.Up(off_, plan_.off);
    io_.Up(records_, plan_.records);
    io_.Up(frame_index_, frames, (size_t)n);
    out_.Resize((size_t)n);
    cand_.Resize((size_t)n * S);
    for (int j = 0; j < 2; ++j) {
      loc_d_[j].Resize((size_t)n);
      flags_d_[j].Resize(std::max<size_t>(total, 1));
    }
    io_.FlushUp(stream_.get());
    RansacArgs ra{};
    ra.frames = frames_.ptr;
    ra.off = off_.ptr;
    ra.records = reinterpret_cast<const double*>(records_.ptr);
    ra.frame_index = frame_index_.ptr;
    ra.cand = cand_.ptr;
    ra.tau2 = lo.threshold_px * lo.threshold_px;
    ra.seed = lo.seed;
    ra.S = S;
    SelectArgs sa{};
    sa.frames = frames_.ptr;
    sa.off = off_.ptr;
    sa.records = ra.records;
    sa.frame_index = frame_index_.ptr;
    sa.cand = cand_.ptr;
    sa.lm = out_.ptr;
    sa.out = loc_d_[0].ptr;
    sa.flags = flags_d_[0].ptr;
    sa.tau2 = ra.tau2;
    sa.seed = lo.seed;
    sa.S = S;
    sa.min_inliers = lo.min_inliers;
    sa.post = 0;
    timer_.Start(stream_.get());
    hipLaunchKernelGGL(k_pose_ransac, dim3((unsigned)((size_t)n * S)), dim3(kPoseThreads), 0, stream_.get(), ra);
    SG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pose_select, dim3((unsigned)n), dim3(kPoseThreads), 0, stream_.get(), sa);
    SG_HIP_CHECK(hipGetLastError());
    if (refine) {
      // the polish reads the PoseFrame array the launch above rewrote: run = 1 for exactly the SG_LOC_OK frames
      LaunchLm(n, lo.range, o);
      sa.out = loc_d_[1].ptr;
      sa.flags = flags_d_[1].ptr;
      sa.post = 1;
      hipLaunchKernelGGL(k_pose_select, dim3((unsigned)n), dim3(kPoseThreads), 0, stream_.get(), sa);
      SG_HIP_CHECK(hipGetLastError());
    }
    timer_.Stop(stream_.get());
    for (int j = 0; j < (refine ? 2 : 1); ++j) {
      loc_h_[j].resize((size_t)n);
      flags_h_[j].resize(total);
      io_.Down(loc_h_[j].data(), loc_d_[j].ptr, (size_t)n * sizeof(LocOut));
      io_.Down(flags_h_[j].data(), flags_d_[j].ptr, total * sizeof(int32_t));
    }
    if (refine) {
      out_h_.resize((size_t)n);
      io_.Down(out_h_.data(), out_.ptr, (size_t)n * sizeof(PoseOut));
    }
    io_.FinishDown(stream_.get());
    timer_.Read();
    for (int i = 0; i < n; ++i) {
      if (!plan_.frames[i].run) continue;   // (its result was not written)
      const LocOut& w = loc_h_[0][i];
      SG_REQUIRE(w.status == SG_LOC_OK || w.status == SG_LOC_NO_MODEL || w.status == SG_LOC_FEW_INLIERS, SG_EDEVICE,
                 "localization status out of range");
      SG_REQUIRE(w.num_obs == res[i].num_obs, SG_EDEVICE, "localization result of another frame");
      sg_localize_result& r = res[i];
      r.status = w.status;
      r.models = w.models;
      if (w.status == SG_LOC_NO_MODEL) continue;
      SG_REQUIRE(w.h >= 0 && w.h < H && w.inliers >= 0 && w.inliers <= w.num_obs, SG_EDEVICE,
                 "localization winner out of range");
      r.best_hypothesis = w.h;
      std::memcpy(r.best_sample, w.sample, sizeof(r.best_sample));
      std::memcpy(r.q, w.q, sizeof(r.q));
      std::memcpy(r.t, w.t, sizeof(r.t));
      r.ransac_cost = w.cost;
      const LocOut* fin = &w;
      if (refine && w.status == SG_LOC_OK) {
        Summarize(i);
        const LocOut& p = loc_h_[1][i];
        SG_REQUIRE(p.status == SG_LOC_OK && p.num_obs == w.num_obs && p.inliers >= 0 && p.inliers <= p.num_obs,
                   SG_EDEVICE, "localization result of another frame after the polish");
        // not worse, in loc_before's order: the cost, then the inlier count, then the inliers' sum of squares
        const bool not_worse = p.cost != w.cost ? p.cost < w.cost
                               : p.inliers != w.inliers ? p.inliers > w.inliers : p.sumsq <= w.sumsq;
        if (sums_[i].ok && not_worse) {
          use_post[i] = 1;
          fin = &p;
        }
      }
      r.refined = use_post[i];
      r.num_inliers = fin->inliers;
      r.msac_cost = fin->cost;
      r.inlier_rms_px = fin->inliers > 0 ? std::sqrt(fin->sumsq / fin->inliers) : 0.0;
    }
  }
  // write-back only after every frame's result has been checked: a failed call changes nothing
  if (obs_inlier)
    for (int32_t j = 0; j < m->num_obs; ++j) obs_inlier[j] = -1;
  for (int i = 0; i < n; ++i) {
    solved[i] = res[i].status == SG_LOC_OK;
    if (!solved[i]) continue;
    const int j = use_post[i];
    const double* q = j ? out_h_[i].q : res[i].q;
    const double* t = j ? out_h_[i].t : res[i].t;
    std::memcpy(m->q + 4 * (size_t)frames[i], q, 4 * sizeof(double));
    std::memcpy(m->t + 3 * (size_t)frames[i], t, 3 * sizeof(double));
    if (obs_inlier)
      for (int32_t r = plan_.off[i]; r < plan_.off[i + 1]; ++r) obs_inlier[plan_.obs[r]] = flags_h_[j][r];
  }
  if (results)
    for (int i = 0; i < n; ++i) results[i] = res[i];
  if (summaries)
    for (int i = 0; i < n; ++i) summaries[i] = sums_[i];
}

}  // namespace sg
