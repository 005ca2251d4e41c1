// retrieve.hip — keyframe retrieval: one frame's descriptors against every keyframe of a device-resident database in
// one call (sg_matcher_db_*, include/slamgpu.h).  Three launches serve the whole database:
//   k_retrieve_slices       hamming.hip's slice body (ham_slice, hamming_tile.h) with the train side segmented:
//                           blockIdx.y walks the host-planned work list of (set, first, count) slices
//                           (retrieve_plan.h), blockIdx.x the groups of 256 queries.  The partial written per (item,
//                           query) is the slice's pair of packed keys rebased to the index within the set, so a
//                           smaller key is a smaller (distance, index in the set).
//   k_retrieve_merge_claim  per (set, query): the set's slices combined in slice order (best = min key, second = the
//                           multiset's second key), the acceptance rule, and one 32-bit atomicMin of
//                           (best_dist << 22) | query on the claim slot of the best descriptor.  Keys are distinct, so
//                           the minimum does not depend on the order of arrival.
//   k_retrieve_resolve      per (set, query): a candidate whose key stands in its claim slot is matched; the per-set
//                           score is a ballot's popcount added with an integer atomic, so it is exact.
// The claim array (one word per database descriptor) is set to all ones and the scores to zero on the stream before the
// three launches.  Everything is integer; a set's cells depend on the query, the options and its own descriptors only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "common.h"
#include "dbuf.h"
#include "hamming_tile.h"
#include "matcher_handle.h"
#include "retrieve_plan.h"

namespace sg {

namespace {

static_assert(kRetrieveQ == kHmQ && kRetrieveTile == kHmTile, "the planner's shapes are the kernel's");

// The slice kernel: the slice comes from the work list, it = (set, first, count, base).
__global__ __launch_bounds__(kHmThreads) void k_retrieve_slices(const uint16_t* __restrict__ qb, int nq,
                                                                const uint16_t* __restrict__ tb,
                                                                const int4* __restrict__ items,
                                                                uint2* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) unsigned char tile[kHmTile * kHmPitch];
  __shared__ unsigned red[4][64][2];
  const int4 it = items[blockIdx.y];
  const int first = __builtin_amdgcn_readfirstlane(it.y), cnt = __builtin_amdgcn_readfirstlane(it.z);   // cnt >= 1
  const int j0 = __builtin_amdgcn_readfirstlane(it.w);
  const HamSliceKeys r = ham_slice(qb, nq, tb, j0, cnt, blockIdx.x, tile, red);
  if (!r.write) return;
  // slice index -> index within the set (first + index < 2^16: no carry into the distance bits)
  unsigned k1 = r.k1, k2 = r.k2;
  if (k1 != kBest2Inf) k1 += (unsigned)first;
  if (k2 != kBest2Inf) k2 += (unsigned)first;
  part[(size_t)blockIdx.y * nq + r.q] = make_uint2(k1, k2);
}

// sets[s] = (item0, nitems, offset, n).  cell[s nq + i] = (best index within the set, best distance) of a candidate,
// else (-1, -1).  Sets without work items (empty, skipped) are not touched: the host knows their rows.
__global__ __launch_bounds__(kRetrieveQ) void k_retrieve_merge_claim(const uint2* __restrict__ part,
                                                                     const int4* __restrict__ sets, int nq,
                                                                     int max_dist, int ratio_percent,
                                                                     int2* __restrict__ cell,
                                                                     unsigned* __restrict__ claim) {
  const int s = blockIdx.y;
  const int4 rec = sets[s];
  const int i = blockIdx.x * kRetrieveQ + threadIdx.x;
  if (rec.y == 0 || i >= nq) return;
  unsigned m1 = kBest2Inf, m2 = kBest2Inf;
  for (int u = 0; u < rec.y; ++u) {   // slice order = index order within the set
    const uint2 p = part[(size_t)(rec.x + u) * nq + i];
    Best2Merge(m1, m2, p.x, p.y);
  }
  // n >= 1, so m1 is a key: (2 h << 22) | index; m2 is one only with n >= 2
  const int bd = (int)(m1 >> (kKeyShift + 1)), bi = (int)(m1 & kBest2IndexMask);
  const int sd = m2 == kBest2Inf ? -1 : (int)(m2 >> (kKeyShift + 1));
  const bool ok = bd <= max_dist && (sd < 0 || 100 * bd <= ratio_percent * sd);
  cell[(size_t)s * nq + i] = ok ? make_int2(bi, bd) : make_int2(-1, -1);
  if (ok) atomicMin(&claim[rec.z + bi], ((unsigned)bd << kRetrieveClaimShift) | (unsigned)i);
}

__global__ __launch_bounds__(kRetrieveQ) void k_retrieve_resolve(int2* __restrict__ cell,
                                                                 const int4* __restrict__ sets, int nq,
                                                                 const unsigned* __restrict__ claim,
                                                                 int32_t* __restrict__ score) {
  const int s = blockIdx.y;
  const int4 rec = sets[s];
  if (rec.y == 0) return;   // the whole workgroup
  const int i = blockIdx.x * kRetrieveQ + threadIdx.x;
  bool won = false;
  if (i < nq) {
    const int2 c = cell[(size_t)s * nq + i];
    if (c.x >= 0) {
      won = claim[rec.z + c.x] == (((unsigned)c.y << kRetrieveClaimShift) | (unsigned)i);
      if (!won) cell[(size_t)s * nq + i] = make_int2(-1, -1);   // no fall-back to a second choice
    }
  }
  const unsigned long long b = __ballot(won);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&score[s], (int32_t)__popcll(b));
}

}  // namespace

class KeyframeDb {
 public:
  KeyframeDb(const sg_device_options& d, hipStream_t stream) : dev_(d), stream_(stream) {
    SG_HIP_CHECK(hipSetDevice(dev_.device));
    SG_HIP_CHECK(hipEventCreate(&e0_));
    SG_HIP_CHECK(hipEventCreate(&e1_));
  }
  ~KeyframeDb() {
    (void)hipSetDevice(dev_.device);
    (void)hipStreamSynchronize(stream_);
    if (e0_) (void)hipEventDestroy(e0_);
    if (e1_) (void)hipEventDestroy(e1_);
  }

  const RetrieveDb& db() const { return db_; }

  int32_t Add(const uint64_t* desc, int32_t n) {
    RetrieveDb next = db_;
    const int32_t id = DbAppend(&next, desc, n);   // every argument error, before the device is touched
    SG_HIP_CHECK(hipSetDevice(dev_.device));
    const size_t old = (size_t)db_.total(), need = (size_t)next.total();
    const size_t cap = (size_t)DbCapacity((int64_t)(desc_.cap / 4), (int64_t)need);
    if (4 * cap > desc_.cap) {
      // grow: the old contents move by a device-to-device copy on the stream; the old buffer is freed after it
      DBuf<uint64_t> grown;
      grown.Reserve(4 * cap);
      if (old) SG_HIP_CHECK(hipMemcpyAsync(grown.ptr, desc_.ptr, 32 * old, hipMemcpyDeviceToDevice, stream_));
      SG_HIP_CHECK(hipStreamSynchronize(stream_));
      std::swap(grown.ptr, desc_.ptr);
      std::swap(grown.cap, desc_.cap);
    }
    if (n) SG_HIP_CHECK(hipMemcpyAsync(desc_.ptr + 4 * old, desc, 32 * (size_t)n, hipMemcpyHostToDevice, stream_));
    SG_HIP_CHECK(hipStreamSynchronize(stream_));   // the caller's array is free on return
    db_ = std::move(next);
    return id;
  }

  void Clear() { db_ = RetrieveDb{}; }   // the device buffer keeps its capacity

  void Query(const uint64_t* query, int32_t nq, const sg_retrieve_options* o, const uint8_t* skip, int32_t* score,
             int32_t k, int32_t* top_set, int32_t* top_score, int32_t* match, int32_t* match_dist) {
    RetrievePlan plan;
    PlanQuery(db_, query, nq, o, skip, score, k, top_set, top_score, &plan);
    const int32_t S = plan.S;
    ms_ = 0.0;
    if (plan.launch) {
      SG_HIP_CHECK(hipSetDevice(dev_.device));
      const size_t nitems = plan.items.size();
      q_.Resize(4 * (size_t)nq);
      SG_HIP_CHECK(hipMemcpyAsync(q_.ptr, query, 32 * (size_t)nq, hipMemcpyHostToDevice, stream_));
      table_.assign((const int32_t*)plan.sets.data(), (const int32_t*)plan.sets.data() + 4 * (size_t)S);
      table_.insert(table_.end(), (const int32_t*)plan.items.data(), (const int32_t*)plan.items.data() + 4 * nitems);
      dtable_.Upload(table_, stream_);
      part_.Resize(2 * nitems * (size_t)nq);
      cell_.Resize(2 * (size_t)S * nq);
      claim_.Resize((size_t)db_.total());
      dscore_.Resize((size_t)S);
      const int4* dsets = (const int4*)dtable_.ptr;
      const int4* ditems = dsets + S;
      SG_HIP_CHECK(hipEventRecord(e0_, stream_));
      SG_HIP_CHECK(hipMemsetAsync(claim_.ptr, 0xFF, 4 * (size_t)db_.total(), stream_));
      SG_HIP_CHECK(hipMemsetAsync(dscore_.ptr, 0, 4 * (size_t)S, stream_));
      hipLaunchKernelGGL(k_retrieve_slices, dim3(plan.qgroups, (unsigned)nitems), dim3(kHmThreads), 0, stream_,
                         (const uint16_t*)q_.ptr, nq, (const uint16_t*)desc_.ptr, ditems, (uint2*)part_.ptr);
      hipLaunchKernelGGL(k_retrieve_merge_claim, dim3(plan.qgroups, S), dim3(kRetrieveQ), 0, stream_,
                         (const uint2*)part_.ptr, dsets, nq, o->max_dist, o->ratio_percent, (int2*)cell_.ptr,
                         (unsigned*)claim_.ptr);
      hipLaunchKernelGGL(k_retrieve_resolve, dim3(plan.qgroups, S), dim3(kRetrieveQ), 0, stream_, (int2*)cell_.ptr,
                         dsets, nq, (const unsigned*)claim_.ptr, dscore_.ptr);
      SG_HIP_CHECK(hipEventRecord(e1_, stream_));
      SG_HIP_CHECK(hipGetLastError());
      SG_HIP_CHECK(hipMemcpyAsync(score, dscore_.ptr, 4 * (size_t)S, hipMemcpyDeviceToHost, stream_));
      SG_HIP_CHECK(hipStreamSynchronize(stream_));
      float t = 0.f;
      SG_HIP_CHECK(hipEventElapsedTime(&t, e0_, e1_));
      ms_ = t;
    } else {
      std::fill(score, score + S, 0);
    }
    for (int32_t s = 0; s < S; ++s)
      if (skip && skip[s]) score[s] = -1;
    RankSets(score, skip, S, o->min_score, k, top_set, top_score);
    ran_ = true;
    if (!match && !match_dist) return;
    // only the rows of the ranked sets come back; a ranked set without work items (an empty one, with min_score 0)
    // has a row of -1
    stage_.resize(2 * (size_t)nq);
    for (int32_t r = 0; r < k; ++r) {
      const int32_t s = top_set[r];
      const bool have = plan.launch && s >= 0 && plan.sets[(size_t)s].nitems > 0;
      if (have) {
        SG_HIP_CHECK(hipMemcpyAsync(stage_.data(), cell_.ptr + 2 * (size_t)s * nq, 8 * (size_t)nq,
                                    hipMemcpyDeviceToHost, stream_));
        SG_HIP_CHECK(hipStreamSynchronize(stream_));
      }
      for (size_t i = 0; i < (size_t)nq; ++i) {
        if (match) match[(size_t)r * nq + i] = have ? stage_[2 * i] : -1;
        if (match_dist) match_dist[(size_t)r * nq + i] = have ? stage_[2 * i + 1] : -1;
      }
    }
  }

  double LastMs() const {
    SG_REQUIRE(ran_, SG_EINVAL, "no query has run");
    return ms_;
  }

 private:
  sg_device_options dev_;
  hipStream_t stream_;
  hipEvent_t e0_ = nullptr, e1_ = nullptr;
  RetrieveDb db_;
  DBuf<uint64_t> desc_, q_;
  DBuf<int32_t> dtable_, part_, cell_, claim_, dscore_;
  std::vector<int32_t> table_, stage_;
  double ms_ = 0.0;
  bool ran_ = false;
};

void DeleteKeyframeDb(KeyframeDb* db) { delete db; }

namespace {

KeyframeDb& Db(sg_matcher* m) {
  SG_REQUIRE(m, SG_EINVAL, "null handle");
  if (!m->db) m->db = new KeyframeDb(m->dev, m->stream);
  return *m->db;
}

}  // namespace

}  // namespace sg

extern "C" {

void sg_retrieve_options_default(sg_retrieve_options* o) {
  if (!o) return;
  o->max_dist = 64;
  o->ratio_percent = 80;
  o->min_score = 1;
}

int sg_matcher_db_add(sg_matcher* m, const uint64_t* desc, int32_t n, int32_t* set_id) {
  SG_CAPI_BEGIN
  SG_REQUIRE(m, SG_EINVAL, "null handle");
  if (!m->db) {   // the argument errors come before the device is touched, also on a handle without a database
    sg::RetrieveDb probe;
    sg::DbAppend(&probe, desc, n);
  }
  const int32_t id = sg::Db(m).Add(desc, n);
  if (set_id) *set_id = id;
  SG_CAPI_END
}

int sg_matcher_db_clear(sg_matcher* m) {
  SG_CAPI_BEGIN
  SG_REQUIRE(m, SG_EINVAL, "null handle");
  if (m->db) m->db->Clear();
  SG_CAPI_END
}

int sg_matcher_db_count(const sg_matcher* m, int32_t* num_sets, int64_t* num_descriptors) {
  SG_CAPI_BEGIN
  SG_REQUIRE(m, SG_EINVAL, "null handle");
  if (num_sets) *num_sets = m->db ? m->db->db().sets() : 0;
  if (num_descriptors) *num_descriptors = m->db ? m->db->db().total() : 0;
  SG_CAPI_END
}

int sg_matcher_db_query(sg_matcher* m, const uint64_t* query, int32_t nq, const sg_retrieve_options* options,
                        const uint8_t* skip, int32_t* score, int32_t k, int32_t* top_set, int32_t* top_score,
                        int32_t* match, int32_t* match_dist) {
  SG_CAPI_BEGIN
  SG_REQUIRE(m, SG_EINVAL, "null handle");
  if (!m->db) {   // an empty database: the planner's checks and the empty answers, without a device
    sg::RetrievePlan plan;
    sg::PlanQuery(sg::RetrieveDb{}, query, nq, options, skip, score, k, top_set, top_score, &plan);
    for (int32_t r = 0; r < k; ++r) top_set[r] = top_score[r] = -1;
    for (size_t c = 0; c < (size_t)k * nq; ++c) {
      if (match) match[c] = -1;
      if (match_dist) match_dist[c] = -1;
    }
  } else {
    m->db->Query(query, nq, options, skip, score, k, top_set, top_score, match, match_dist);
  }
  SG_CAPI_END
}

int sg_matcher_db_query_ms(sg_matcher* m, double* kernel_ms) {
  SG_CAPI_BEGIN
  SG_REQUIRE(m && kernel_ms, SG_EINVAL, "null argument");
  SG_REQUIRE(m->db, SG_EINVAL, "no query has run");
  *kernel_ms = m->db->LastMs();
  SG_CAPI_END
}

}  // extern "C"
