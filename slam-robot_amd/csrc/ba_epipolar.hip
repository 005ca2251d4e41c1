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
// hamming.hip's packed-key rule, key = (distance << 22) | b index within the pair; the four waves' answers meet in
// LDS.  A tile's tail is padded with EpiPadB: an infinite nb with a NaN x_b, whose r is NaN, so the gate's comparison
// is false and a padded entry is never counted.
//
// k_epi_merge: one thread per a keypoint merges its slices in slice order and sums their candidate counts.
//
// Every count is known on the host: no device counter, no atomic.  The keys of one a keypoint are distinct (the b
// indices are), so the smallest and the second smallest of its keys do not depend on the order in which they are taken
// or merged, and neither does an integer count.  A pair's records come from its own pair record and keypoints alone, so
// its results depend neither on its position in the call nor on the run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "ba_epipolar.h"
#include "epipolar_math.h"

namespace sg {

namespace {

constexpr int kEpiThreads = 256;
constexpr unsigned kEpiKeyInf = 0xFFFFFFFFu;
constexpr unsigned kEpiPosMask = (1u << kEpiKeyShift) - 1;
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

__device__ __forceinline__ void epi_take(unsigned key, unsigned& m1, unsigned& m2) {
  m2 = min(m2, max(m1, key));   // the median of (m1, key, m2) with m1 <= m2: the second smallest
  m1 = min(m1, key);
}

__device__ __forceinline__ void epi_merge(unsigned& m1, unsigned& m2, unsigned o1, unsigned o2) {
  const unsigned n2 = min(max(m1, o1), min(m2, o2));
  m1 = min(m1, o1);
  m2 = n2;
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
  unsigned m1 = kEpiKeyInf, m2 = kEpiKeyInf;
  int wn = 0;
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
            const unsigned h = __popc(q0.x ^ d0.x) + __popc(q0.y ^ d0.y) + __popc(q0.z ^ d0.z) + __popc(q0.w ^ d0.w) +
                               __popc(q1.x ^ d1.x) + __popc(q1.y ^ d1.y) + __popc(q1.z ^ d1.z) + __popc(q1.w ^ d1.w);
            epi_take((h << kEpiKeyShift) | (unsigned)(it.j0 + t0 + e + u), m1, m2);
            ++wn;
          }
        }
      }
    }
  }
  // the four waves' answers for the same 64 a keypoints meet in LDS; wave 0 merges them in wave order
  if (wave > 0) wpart[wave - 1][lane] = make_uint4(m1, m2, (unsigned)wn, 0u);
  __syncthreads();
  if (wave > 0 || !live) return;
#pragma unroll
  for (int w = 0; w < kEpiWaves - 1; ++w) {
    const uint4 o = wpart[w][lane];
    epi_merge(m1, m2, o.x, o.y);
    wn += (int)o.z;
  }
  a.part[(size_t)it.part0 + lane] = make_uint4(m1, m2, (unsigned)wn, 0u);
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
  const int ns = ch.slices;
  unsigned m1 = kEpiKeyInf, m2 = kEpiKeyInf, wn = 0;
  for (int s0 = 0; s0 < ns; s0 += 8) {   // slice order, eight loads a trip as in k_match_merge
    uint4 p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = a.part[p0 + (size_t)min(s0 + u, ns - 1) * ch.stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (s0 + u >= ns) break;
      epi_merge(m1, m2, p[u].x, p[u].y);
      wn += p[u].z;
    }
  }
  a.out[k] = m1 == kEpiKeyInf ? -1 : (int)(m1 & kEpiPosMask);
  a.out[(size_t)a.KA + k] = m1 == kEpiKeyInf ? -1 : (int)(m1 >> kEpiKeyShift);
  a.out[2 * (size_t)a.KA + k] = m2 == kEpiKeyInf ? -1 : (int)(m2 >> kEpiKeyShift);
  a.out[3 * (size_t)a.KA + k] = (int)wn;
}

}  // namespace

EpipolarSolver::EpipolarSolver(const sg_device_options& dev, hipStream_t stream) : dev_(dev) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw Error(SG_ENODEV, "no HIP device available");
  SG_REQUIRE(dev.device >= 0 && dev.device < ndev, SG_ENODEV, "device ordinal out of range");
  SG_HIP_CHECK(hipSetDevice(dev.device));
  if (stream) {
    stream_ = stream;
  } else {
    SG_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    own_stream_ = true;
  }
}

EpipolarSolver::~EpipolarSolver() {
  for (hipEvent_t e : ev_)
    if (e) (void)hipEventDestroy(e);
  if (own_stream_ && stream_) (void)hipStreamDestroy(stream_);
}

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
  SG_HIP_CHECK(hipSetDevice(dev_.device));
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
  io_.FlushUp(stream_);

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
  if (timing_) {
    for (hipEvent_t& e : ev_)
      if (!e) SG_HIP_CHECK(hipEventCreate(&e));
    SG_HIP_CHECK(hipEventRecord(ev_[0], stream_));
  }
  hipLaunchKernelGGL(k_epi_prep, dim3((unsigned)plan.prep.size()), dim3(kEpiThreads), 0, stream_, pa);
  SG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_epi_window, dim3((unsigned)plan.items.size()), dim3(kEpiThreads), 0, stream_, wa);
  SG_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_epi_merge, dim3((unsigned)plan.chunks.size()), dim3(kEpiChunk), 0, stream_, ma);
  SG_HIP_CHECK(hipGetLastError());
  if (timing_) SG_HIP_CHECK(hipEventRecord(ev_[1], stream_));
  std::vector<int32_t> out_h(4 * KA);
  io_.Down(out_h.data(), out_.ptr, out_h.size() * sizeof(int32_t));
  io_.FinishDown(stream_);
  kernel_ms_ = 0.0;
  if (timing_) {
    float ms = 0.f;
    SG_HIP_CHECK(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
    kernel_ms_ = ms;
  }
  for (int i = 0; i < n; ++i) {
    const int32_t nb = b_offset[i + 1] - b_offset[i];
    for (int32_t k = a_offset[i]; k < a_offset[i + 1]; ++k) {
      int32_t &bk = out_h[k], &bd = out_h[KA + k], &sd = out_h[2 * KA + k], &wn = out_h[3 * KA + k];
      if (!plan.live[i]) {   // no kernel wrote these: the empty answers
        bk = bd = sd = -1;
        wn = 0;
        continue;
      }
      SG_REQUIRE(wn >= 0 && wn <= nb && (wn == 0) == (bk < 0) && (wn < 2) == (sd < 0), SG_EDEVICE,
                 "candidate count out of range");
      SG_REQUIRE(bk < 0 ? bk == -1 && bd == -1 : bk < nb && bd >= 0 && bd <= 256, SG_EDEVICE,
                 "best match out of range");
      SG_REQUIRE(sd < 0 ? sd == -1 : sd >= bd && sd <= 256, SG_EDEVICE, "second distance out of range");
    }
  }
  // outputs only after every value has been checked: a failing call writes nothing
  std::memcpy(best_kp, out_h.data(), KA * sizeof(int32_t));
  std::memcpy(best_dist, out_h.data() + KA, KA * sizeof(int32_t));
  std::memcpy(second_dist, out_h.data() + 2 * KA, KA * sizeof(int32_t));
  std::memcpy(num_candidates, out_h.data() + 3 * KA, KA * sizeof(int32_t));
}

}  // namespace sg
