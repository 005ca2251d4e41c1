// ba_match.hip — match by projection: sg_slam_match_by_projection.
//
// Which of the listed points does each listed frame see, and which keypoint is which point?  Three launches on the
// handle's stream, no host round trip between them (match_plan.h: what they read and the launch shapes).
//
// k_match_project: one thread per (listed frame, position of points[]), project_blocks x n workgroups of 256.  Project
// of project_math.h in fp64, the culls of the contract (behind the camera, not finite, outside the image, already
// observed: one bit of the planner's mask), and a per-wave compaction of the survivors into the frame's list: a ballot,
// one atomic add of the wave's count on the frame's counter, and each surviving lane writes u, v, its position and the
// point's 32-byte descriptor at the wave's base plus its rank in the ballot.  The order of a frame's list therefore
// varies from run to run; nothing after it depends on the order (below).
//
// k_match_window: one workgroup of 256 per (chunk of 64 keypoints, slice of kMatchSlice survivors).  Lane l of every wave
// keeps keypoint l's pixel and descriptor in registers; the slice goes through LDS a tile of 256 at a time, each wave
// scores its quarter of the tile, and in the scoring loop every lane reads the same entry (a broadcast: no bank
// conflict), four entries a trip.  The fp64 distance test comes first; the popcounts run only for entries inside the
// window.  best and second follow best2.h's packed-key rule, key = (distance << 22) | position; the four waves'
// answers meet in LDS.  Splitting the survivors over the waves (not the keypoints) keeps each wave's serial walk at a
// quarter of the slice and puts four times as many workgroups on the chip, which is what a one-frame call needs: it
// is bound by the latency of that walk, not by throughput.  The slice count comes from np alone, so the grid is
// known on the host; a workgroup whose slice starts at or beyond the frame's survivor count (read from the device
// counter) exits.
//
// k_match_merge: one thread per keypoint merges the slices that exist for its frame, in slice order, and sums their
// window sizes.
//
// Order independence: the keys of one keypoint are distinct (positions are), so best2.h's rule gives the same best
// and second whatever the order of a frame's list, and an integer count does not depend on it either.  Every output
// is such a min, second-min or count over the frame's survivor set, which is itself fixed by the arithmetic of Project
// on the inputs: the results are reproducible bit for bit although the lists are not.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "ba_match.h"
#include "best2.h"
#include "project_math.h"

namespace sg {

namespace {

constexpr int kMatchThreads = 256;
constexpr int kMatchWaves = kMatchThreads / 64;
constexpr int kMatchShare = kMatchTile / kMatchWaves;   // a wave's entries of a tile
static_assert(kMatchChunk == 64 && kMatchTile == kMatchThreads, "one keypoint per lane and one tile entry per thread");
static_assert(kMatchShare % 4 == 0, "the scoring loop reads four entries a trip");

struct MatchProjectArgs {
  const MatchFrame* frames;   // [n]
  const double* X;            // [4 np]
  const uint4* point_desc;    // [2 np]
  const uint32_t* excl;       // [n * words]
  int32_t* count;             // [n], zero at launch
  double2* surv_uv;           // [n * np]
  uint4* surv_desc;           // [2 n * np]
  int32_t* surv_pos;          // [n * np]
  double width, height;       // 0, 0: no bound
  int32_t np, words, blocks;
};

__global__ __launch_bounds__(kMatchThreads) void k_match_project(MatchProjectArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int slot = blockIdx.x / a.blocks;   // (a flat grid: the frame count may exceed a grid's y range)
  const int j = (blockIdx.x % a.blocks) * kMatchThreads + tid;
  bool ok = false;
  double uv[2] = {0.0, 0.0};
  if (j < a.np) {
    const MatchFrame& f = a.frames[slot];
    const double q[4] = {f.q[0], f.q[1], f.q[2], f.q[3]}, t[3] = {f.t[0], f.t[1], f.t[2]};
    const double k[7] = {f.k[0], f.k[1], f.k[2], f.k[3], f.k[4], f.k[5], f.k[6]};
    const double X[4] = {a.X[4 * (size_t)j], a.X[4 * (size_t)j + 1], a.X[4 * (size_t)j + 2], a.X[4 * (size_t)j + 3]};
    ok = Project(q, t, k, X, uv);
    ok = ok && isfinite(uv[0]) && isfinite(uv[1]);
    if (a.width > 0.0) ok = ok && uv[0] >= 0.0 && uv[0] < a.width && uv[1] >= 0.0 && uv[1] < a.height;
    ok = ok && ((a.excl[(size_t)slot * a.words + (j >> 5)] >> (j & 31)) & 1u) == 0;
  }
  const unsigned long long b = __ballot(ok);
  if (b == 0) return;   // (the whole wave)
  int base = 0;
  if (lane == __ffsll(b) - 1) base = atomicAdd(a.count + slot, __popcll(b));
  base = __shfl(base, __ffsll(b) - 1);
  if (!ok) return;
  // at most np survivors per frame, so base + rank < np
  const size_t at = (size_t)slot * a.np + base + __popcll(b & ((1ull << lane) - 1ull));
  a.surv_uv[at] = make_double2(uv[0], uv[1]);
  a.surv_desc[2 * at] = a.point_desc[2 * (size_t)j];
  a.surv_desc[2 * at + 1] = a.point_desc[2 * (size_t)j + 1];
  a.surv_pos[at] = j;
}

struct MatchWindowArgs {
  const MatchChunk* chunks;
  const int32_t* count;       // [n] survivors per listed frame
  const double2* kp_xy;       // [K]
  const uint4* kp_desc;       // [2 K]
  const double2* surv_uv;
  const uint4* surv_desc;
  const int32_t* surv_pos;
  uint4* part;                // [slices * K]
  double r2;
  int32_t np, K, slices;
};

__global__ __launch_bounds__(kMatchThreads) void k_match_window(MatchWindowArgs a) {
  __shared__ double2 suv[kMatchTile];
  __shared__ uint4 sdesc[kMatchTile][2];
  __shared__ int32_t spos[kMatchTile];
  __shared__ uint4 wpart[kMatchWaves - 1][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const MatchChunk ch = a.chunks[blockIdx.x / a.slices];
  const int slice = blockIdx.x % a.slices;
  const int total = a.count[ch.slot];
  const int s0 = slice * kMatchSlice;
  if (s0 >= total) return;   // (the whole workgroup) the frame has no such slice
  const int s1 = min(total, s0 + kMatchSlice);
  const bool live = lane < ch.count;
  const int kp = ch.kp0 + (live ? lane : 0);   // (an idle lane reads the chunk's first keypoint and writes nothing)
  const double2 xy = a.kp_xy[kp];
  const uint4 d0 = a.kp_desc[2 * (size_t)kp], d1 = a.kp_desc[2 * (size_t)kp + 1];
  const size_t fb = (size_t)ch.slot * a.np;
  unsigned m1 = kBest2Inf, m2 = kBest2Inf, wn = 0;
  for (int t0 = s0; t0 < s1; t0 += kMatchTile) {
    const int tc = min(kMatchTile, s1 - t0);
    __syncthreads();   // the previous tile has been read
    {
      const bool in = tid < tc;
      const size_t at = fb + t0 + (in ? tid : 0);
      // the tile's tail is padded with pixels at infinity: in no window, so the scoring loop runs in whole fours
      suv[tid] = in ? a.surv_uv[at] : make_double2(INFINITY, INFINITY);
      if (in) {
        sdesc[tid][0] = a.surv_desc[2 * at];
        sdesc[tid][1] = a.surv_desc[2 * at + 1];
        spos[tid] = a.surv_pos[at];
      }
    }
    __syncthreads();
    // each wave scores its quarter of the tile against the chunk's 64 keypoints; every lane reads entries
    // e .. e + 3 (broadcasts), four distances in flight
    const int e1 = min(tc, (wave + 1) * kMatchShare);
    for (int e = wave * kMatchShare; e < e1; e += 4) {
      double dist2[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double2 p = suv[e + u];
        const double du = p.x - xy.x, dv = p.y - xy.y;
        dist2[u] = __dadd_rn(__dmul_rn(du, du), __dmul_rn(dv, dv));   // (no contraction: the contract's rounding)
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (dist2[u] <= a.r2) {   // (false for a non-finite keypoint and for the padding)
          const uint4 q0 = sdesc[e + u][0], q1 = sdesc[e + u][1];
          const unsigned h = Hamming256(q0, q1, d0, d1);
          Best2Take((h << kMatchKeyShift) | (unsigned)spos[e + u], m1, m2);
          ++wn;
        }
      }
    }
  }
  // the four waves' answers for the same 64 keypoints meet in LDS
  if (!Best2MeetWaves<kMatchWaves>(wpart, wave, lane, m1, m2, wn) || !live) return;
  a.part[(size_t)slice * a.K + kp] = make_uint4(m1, m2, wn, 0u);
}

struct MatchMergeArgs {
  const MatchChunk* chunks;
  const int32_t* count;
  const uint4* part;
  const int32_t* points;   // [np] position -> map index
  int32_t* out;            // [4 K]
  int32_t K;
};

__global__ __launch_bounds__(kMatchChunk) void k_match_merge(MatchMergeArgs a) {
  const MatchChunk ch = a.chunks[blockIdx.x];
  if ((int)threadIdx.x >= ch.count) return;
  const int kp = ch.kp0 + threadIdx.x;
  const int ns = (a.count[ch.slot] + kMatchSlice - 1) / kMatchSlice;   // the slices k_match_window wrote
  unsigned m1, m2, wn;
  Best2MergeSlices(a.part, (size_t)kp, (size_t)a.K, ns, m1, m2, wn);
  Best2Result r = Best2Decode(m1, m2, wn);
  if (r.index >= 0) r.index = a.points[r.index];   // position in points[] -> map index
  Best2Store(a.out, (size_t)a.K, (size_t)kp, r);
}

}  // namespace

void MatchSolver::Run(const MatchPlan& plan, const double* kp_xy, const uint64_t* kp_desc, const int32_t* points,
                      const uint64_t* point_desc, const sg_match_options& o, int32_t* best_point, int32_t* best_dist,
                      int32_t* second_dist, int32_t* num_candidates, int32_t* projected) {
  SG_REQUIRE(plan.launch && kp_xy && kp_desc && points && point_desc && best_point && best_dist && second_dist &&
                 num_candidates && projected,
             SG_EINVAL, "bad argument");
  const int n = plan.n, np = plan.np, K = plan.K, S = plan.slices;
  const size_t nchunk = plan.chunks.size();
  // (n np <= 2^22 and K <= 2^20 keep both flat grids far below 2^24 workgroups)
  SG_REQUIRE(n > 0 && S > 0 && nchunk > 0 && (size_t)plan.project_blocks * n < (1u << 24) && nchunk * S < (1u << 24),
             SG_EINVAL, "launch shape out of range");
  stream_.Bind();
  io_.Begin();
  io_.Up(frames_, plan.frames);
  io_.Up(chunks_, plan.chunks);
  io_.Up(X_, plan.X);
  io_.Up(excl_, plan.excl);
  io_.Up(kp_xy_, kp_xy, 2 * (size_t)K);
  io_.Up(kp_desc_, kp_desc, 4 * (size_t)K);
  io_.Up(point_desc_, point_desc, 4 * (size_t)np);
  io_.Up(points_, points, (size_t)np);
  io_.UpZero(count_, (size_t)n);
  const size_t pairs = (size_t)n * np;
  surv_uv_.Resize(pairs);
  surv_desc_.Resize(2 * pairs);
  surv_pos_.Resize(pairs);
  part_.Resize((size_t)S * K);
  out_.Resize(4 * (size_t)K);
  io_.FlushUp(stream_.get());

  MatchProjectArgs pa{};
  pa.frames = frames_.ptr;
  pa.X = X_.ptr;
  pa.point_desc = reinterpret_cast<const uint4*>(point_desc_.ptr);
  pa.excl = excl_.ptr;
  pa.count = count_.ptr;
  pa.surv_uv = surv_uv_.ptr;
  pa.surv_desc = surv_desc_.ptr;
  pa.surv_pos = surv_pos_.ptr;
  pa.width = (double)o.width;
  pa.height = (double)o.height;
  pa.np = np;
  pa.words = plan.words;
  pa.blocks = plan.project_blocks;
  MatchWindowArgs wa{};
  wa.chunks = chunks_.ptr;
  wa.count = count_.ptr;
  wa.kp_xy = reinterpret_cast<const double2*>(kp_xy_.ptr);
  wa.kp_desc = reinterpret_cast<const uint4*>(kp_desc_.ptr);
  wa.surv_uv = surv_uv_.ptr;
  wa.surv_desc = surv_desc_.ptr;
  wa.surv_pos = surv_pos_.ptr;
  wa.part = part_.ptr;
  wa.r2 = o.radius_px * o.radius_px;
  wa.np = np;
  wa.K = K;
  wa.slices = S;
  MatchMergeArgs ma{};
  ma.chunks = chunks_.ptr;
  ma.count = count_.ptr;
  ma.part = part_.ptr;
  ma.points = points_.ptr;
  ma.out = out_.ptr;
  ma.K = K;
  timer_.Start(stream_.get());
  hipLaunchKernelGGL(k_match_project, dim3((unsigned)(plan.project_blocks * n)), dim3(kMatchThreads), 0, stream_.get(),
                     pa);
  SG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_match_window, dim3((unsigned)(nchunk * S)), dim3(kMatchThreads), 0, stream_.get(), wa);
  SG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_match_merge, dim3((unsigned)nchunk), dim3(kMatchChunk), 0, stream_.get(), ma);
  SG_HIP_CHECK(hipGetLastError());
  timer_.Stop(stream_.get());
  std::vector<int32_t> out_h(4 * (size_t)K), count_h((size_t)n);
  io_.Down(out_h.data(), out_.ptr, out_h.size() * sizeof(int32_t));
  io_.Down(count_h.data(), count_.ptr, count_h.size() * sizeof(int32_t));
  io_.FinishDown(stream_.get());
  timer_.Read();
  for (int i = 0; i < n; ++i)
    SG_REQUIRE(count_h[i] >= 0 && count_h[i] <= np, SG_EDEVICE, "survivor count out of range");
  for (size_t c = 0; c < nchunk; ++c) {
    const MatchChunk& ch = plan.chunks[c];
    for (int32_t k = ch.kp0; k < ch.kp0 + ch.count; ++k) {
      const int32_t bp = out_h[k], bd = out_h[(size_t)K + k], sd = out_h[2 * (size_t)K + k], wn = out_h[3 * (size_t)K + k];
      // (bp is a map index, of which this call knows no bound)
      SG_REQUIRE(Best2ResultOk(bp, bd, sd, wn, INT32_MAX, count_h[ch.slot]), SG_EDEVICE, "match result out of range");
    }
  }
  // outputs only after every value has been checked: a failing call writes nothing
  std::memcpy(best_point, out_h.data(), (size_t)K * sizeof(int32_t));
  std::memcpy(best_dist, out_h.data() + (size_t)K, (size_t)K * sizeof(int32_t));
  std::memcpy(second_dist, out_h.data() + 2 * (size_t)K, (size_t)K * sizeof(int32_t));
  std::memcpy(num_candidates, out_h.data() + 3 * (size_t)K, (size_t)K * sizeof(int32_t));
  std::memcpy(projected, count_h.data(), (size_t)n * sizeof(int32_t));
}

}  // namespace sg
