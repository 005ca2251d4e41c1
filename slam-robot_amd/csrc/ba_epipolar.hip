// ba_epipolar.hip — match along epipolar lines: sg_slam_match_epipolar.
//
// Which keypoint of frame b is the keypoint of frame a, for frame pairs whose poses are known?  Three launches on the
// handle's stream, no host round trip between them (epipolar_plan.h: what they read and the launch shapes; the
// arithmetic is epipolar_math.h's, the one copy the CPU executor runs too).
//
// k_epi_prep: one thread per keypoint of a live pair, a workgroup of 256 per run of the planner's preparation list.
// It writes the keypoint's record once (EpiA: x_a, l, na, g, g.g, g.tr, 4^level; EpiB: x_b, nb, 4^level, f.f, f.tr),
// so the 8-step Newton undistortion runs once per keypoint and not once per candidate.
//
// k_epi_window: one workgroup of 256 per work item (chunk of 64 a keypoints, slice of kEpiSlice b keypoints),
// structured like k_match_window (ba_match.hip).  Lane l of every wave keeps a keypoint l's record and descriptor in
// registers; the slice goes through LDS a tile of 256 at a time, each wave scores its quarter of the tile, and in the
// scoring loop every lane reads the same entry (a broadcast: no bank conflict), four entries a trip.  The gate comes
// first; the depth and parallax tests and the popcounts run only for entries inside it.  best and second follow
// best2.h's packed-key rule, key = (distance << 22) | b index within the pair; the four waves' answers meet in
// LDS.  A tile's tail is padded with EpiPadB: an infinite nb with a NaN x_b, whose r is NaN, so the gate's comparison
// is false and a padded entry is never counted.
//
// k_epi_merge: one thread per a keypoint merges its slices in slice order and sums their candidate counts.
//
// Every count is known on the host: no device counter, no atomic.  The keys of one a keypoint are distinct (the b
// indices are), so best2.h's rule gives the same best and second whatever the order in which they are taken or
// merged, and an integer count does not depend on it either.  A pair's records come from its own pair record and
// keypoints alone, so its results depend neither on its position in the call nor on the run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "ba_epipolar.h"
#include "best2.h"
#include "epipolar_math.h"

namespace sg {

namespace {

constexpr int kEpiThreads = 256;
constexpr int kEpiWaves = kEpiThreads / 64;
constexpr int kEpiShare = kEpiTile / kEpiWaves;   // a wave's entries of a tile
static_assert(kEpiChunk == 64 && kEpiTile == kEpiThreads, "one a keypoint per lane and one tile entry per thread");
static_assert(kEpiPrepRun == kEpiThreads, "one keypoint per thread of k_epi_prep");
static_assert(kEpiShare % 4 == 0, "the scoring loop reads four entries a trip");

struct EpiPrepArgs {
  const EpiPair* pairs;
  const EpiPrepItem* prep;
  const double* a_xy;        // [2 KA]
  const double* b_xy;        // [2 KB]
  const int32_t* a_level;    // [KA] or null
  const int32_t* b_level;    // [KB] or null
  EpiA* a_rec;               // [KA]
  EpiB* b_rec;               // [KB]
};

__global__ __launch_bounds__(kEpiThreads) void k_epi_prep(EpiPrepArgs a) {
  const EpiPrepItem it = a.prep[blockIdx.x];
  if ((int)threadIdx.x >= it.count) return;
  const size_t k = (size_t)it.k0 + threadIdx.x;
  const EpiPair& p = a.pairs[it.pair];
  if (it.side == 0) {
    const double px[2] = {a.a_xy[2 * k], a.a_xy[2 * k + 1]};
    EpiA r;
    EpiPrepA(p, px, a.a_level ? a.a_level[k] : 0, &r);
    a.a_rec[k] = r;
  } else {
    const double px[2] = {a.b_xy[2 * k], a.b_xy[2 * k + 1]};
    EpiB r;
    EpiPrepB(p, px, a.b_level ? a.b_level[k] : 0, &r);
    a.b_rec[k] = r;
  }
}

struct EpiWindowArgs {
  const EpiItem* items;
  const EpiA* a_rec;
  const EpiB* b_rec;
  const uint4* a_desc;   // [2 KA]
  const uint4* b_desc;   // [2 KB]
  uint4* part;           // [partials]
  double tol2, min_parallax;
};

__global__ __launch_bounds__(kEpiThreads) void k_epi_window(EpiWindowArgs a) {
  __shared__ EpiB srec[kEpiTile];
  __shared__ uint4 sdesc[kEpiTile][2];
  __shared__ uint4 wpart[kEpiWaves - 1][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const EpiItem it = a.items[blockIdx.x];
  const bool live = lane < it.acount;
  const size_t ka = (size_t)it.a0 + (live ? lane : 0);   // (an idle lane reads the chunk's first keypoint and writes nothing)
  const EpiA ra = a.a_rec[ka];
  const uint4 d0 = a.a_desc[2 * ka], d1 = a.a_desc[2 * ka + 1];
  unsigned m1 = kBest2Inf, m2 = kBest2Inf, wn = 0;
  for (int t0 = 0; t0 < it.bcount; t0 += kEpiTile) {
    const int tc = min(kEpiTile, it.bcount - t0);
    __syncthreads();   // the previous tile has been read
    {
      const bool in = tid < tc;
      const size_t at = (size_t)it.b0 + t0 + (in ? tid : 0);
      // the tile's tail is padded with records that fail the gate, so the scoring loop runs in whole fours
      srec[tid] = in ? a.b_rec[at] : EpiPadB();
      if (in) {
        sdesc[tid][0] = a.b_desc[2 * at];
        sdesc[tid][1] = a.b_desc[2 * at + 1];
      }
    }
    __syncthreads();
    // each wave scores its quarter of the tile against the chunk's 64 a keypoints; every lane reads entries
    // e .. e + 3 (broadcasts), four gates in flight
    const int e1 = min(tc, (wave + 1) * kEpiShare);
    for (int e = wave * kEpiShare; e < e1; e += 4) {
      bool gate[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) gate[u] = EpiGate(ra, srec[e + u], a.tol2);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (gate[u]) {   // (false for a non-finite keypoint on either side and for the padding)
          const EpiB rb = srec[e + u];
          if (EpiDepth(ra, rb) && (!(a.min_parallax > 0.0) || EpiParallax(ra, rb, a.min_parallax))) {
            const uint4 q0 = sdesc[e + u][0], q1 = sdesc[e + u][1];
            const unsigned h = Hamming256(q0, q1, d0, d1);
            Best2Take((h << kEpiKeyShift) | (unsigned)(it.j0 + t0 + e + u), m1, m2);
            ++wn;
          }
        }
      }
    }
  }
  // the four waves' answers for the same 64 a keypoints meet in LDS
  if (!Best2MeetWaves<kEpiWaves>(wpart, wave, lane, m1, m2, wn) || !live) return;
  a.part[(size_t)it.part0 + lane] = make_uint4(m1, m2, wn, 0u);
}

struct EpiMergeArgs {
  const EpiChunkItem* chunks;
  const uint4* part;
  int32_t* out;   // [4 KA]
  int32_t KA;
};

__global__ __launch_bounds__(kEpiChunk) void k_epi_merge(EpiMergeArgs a) {
  const EpiChunkItem ch = a.chunks[blockIdx.x];
  if ((int)threadIdx.x >= ch.count) return;
  const size_t k = (size_t)ch.a0 + threadIdx.x;
  const size_t p0 = (size_t)ch.part0 + threadIdx.x;
  unsigned m1, m2, wn;
  Best2MergeSlices(a.part, p0, (size_t)ch.stride, ch.slices, m1, m2, wn);
  Best2Store(a.out, (size_t)a.KA, k, Best2Decode(m1, m2, wn));
}

}  // namespace

void EpipolarSolver::Run(const EpipolarPlan& plan, const int32_t* a_offset, const double* a_xy, const uint64_t* a_desc,
                         const int32_t* a_level, const int32_t* b_offset, const double* b_xy, const uint64_t* b_desc,
                         const int32_t* b_level, const sg_epipolar_options& o, int32_t* best_kp, int32_t* best_dist,
                         int32_t* second_dist, int32_t* num_candidates) {
  SG_REQUIRE(plan.launch && a_offset && a_xy && a_desc && b_offset && b_xy && b_desc && best_kp && best_dist &&
                 second_dist && num_candidates && (a_level != nullptr) == plan.levels &&
                 (b_level != nullptr) == plan.levels,
             SG_EINVAL, "bad argument");
  const int n = plan.n;
  const size_t KA = (size_t)plan.KA, KB = (size_t)plan.KB;
  // (KA, KB <= 2^20 and partials <= 2^23 keep the three flat grids far below 2^24 workgroups)
  SG_REQUIRE(n > 0 && KA > 0 && KB > 0 && plan.partials > 0 && plan.partials <= kEpiMaxPartials &&
                 !plan.prep.empty() && !plan.chunks.empty() && plan.prep.size() < (1u << 24) &&
                 plan.items.size() < (1u << 24) && plan.chunks.size() < (1u << 24),
             SG_EINVAL, "launch shape out of range");
  stream_.Bind();
  io_.Begin();
  io_.Up(pairs_, plan.pairs);
  io_.Up(prep_, plan.prep);
  io_.Up(items_, plan.items);
  io_.Up(chunks_, plan.chunks);
  io_.Up(a_xy_, a_xy, 2 * KA);
  io_.Up(b_xy_, b_xy, 2 * KB);
  io_.Up(a_desc_, a_desc, 4 * KA);
  io_.Up(b_desc_, b_desc, 4 * KB);
  if (plan.levels) {
    io_.Up(a_level_, a_level, KA);
    io_.Up(b_level_, b_level, KB);
  }
  a_rec_.Resize(KA);
  b_rec_.Resize(KB);
  part_.Resize((size_t)plan.partials);
  out_.Resize(4 * KA);
  io_.FlushUp(stream_.get());

  EpiPrepArgs pa{};
  pa.pairs = pairs_.ptr;
  pa.prep = prep_.ptr;
  pa.a_xy = a_xy_.ptr;
  pa.b_xy = b_xy_.ptr;
  pa.a_level = plan.levels ? a_level_.ptr : nullptr;
  pa.b_level = plan.levels ? b_level_.ptr : nullptr;
  pa.a_rec = a_rec_.ptr;
  pa.b_rec = b_rec_.ptr;
  EpiWindowArgs wa{};
  wa.items = items_.ptr;
  wa.a_rec = a_rec_.ptr;
  wa.b_rec = b_rec_.ptr;
  wa.a_desc = reinterpret_cast<const uint4*>(a_desc_.ptr);
  wa.b_desc = reinterpret_cast<const uint4*>(b_desc_.ptr);
  wa.part = part_.ptr;
  wa.tol2 = o.tol_px * o.tol_px;
  wa.min_parallax = o.min_parallax;
  EpiMergeArgs ma{};
  ma.chunks = chunks_.ptr;
  ma.part = part_.ptr;
  ma.out = out_.ptr;
  ma.KA = (int32_t)KA;
  timer_.Start(stream_.get());
  hipLaunchKernelGGL(k_epi_prep, dim3((unsigned)plan.prep.size()), dim3(kEpiThreads), 0, stream_.get(), pa);
  SG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_epi_window, dim3((unsigned)plan.items.size()), dim3(kEpiThreads), 0, stream_.get(), wa);
  SG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_epi_merge, dim3((unsigned)plan.chunks.size()), dim3(kEpiChunk), 0, stream_.get(), ma);
  SG_HIP_CHECK(hipGetLastError());
  timer_.Stop(stream_.get());
  std::vector<int32_t> out_h(4 * KA);
  io_.Down(out_h.data(), out_.ptr, out_h.size() * sizeof(int32_t));
  io_.FinishDown(stream_.get());
  timer_.Read();
  for (int i = 0; i < n; ++i) {
    const int32_t nb = b_offset[i + 1] - b_offset[i];
    for (int32_t k = a_offset[i]; k < a_offset[i + 1]; ++k) {
      int32_t &bk = out_h[k], &bd = out_h[KA + k], &sd = out_h[2 * KA + k], &wn = out_h[3 * KA + k];
      if (!plan.live[i]) {   // no kernel wrote these: the empty answers
        bk = bd = sd = -1;
        wn = 0;
        continue;
      }
      SG_REQUIRE(Best2ResultOk(bk, bd, sd, wn, nb, nb), SG_EDEVICE, "match result out of range");
    }
  }
  // outputs only after every value has been checked: a failing call writes nothing
  std::memcpy(best_kp, out_h.data(), KA * sizeof(int32_t));
  std::memcpy(best_dist, out_h.data() + KA, KA * sizeof(int32_t));
  std::memcpy(second_dist, out_h.data() + 2 * KA, KA * sizeof(int32_t));
  std::memcpy(num_candidates, out_h.data() + 3 * KA, KA * sizeof(int32_t));
}

}  // namespace sg
