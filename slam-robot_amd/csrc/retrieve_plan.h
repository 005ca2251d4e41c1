// retrieve_plan.h — the host-only side of the keyframe descriptor database (sg_matcher_db_*, retrieve.hip): the
// database's bookkeeping (set offsets, caps, capacity growth), the slice work list and launch shapes of a query, every
// SG_EINVAL case of the contract, the ranking rule, and a plain CPU executor of the whole contract.  Pure functions of
// their arguments (no HIP, no environment, no I/O), so a CPU test recomputes them by brute force
// (tests/native/retrieve_plan_check.cpp).
//
// A query runs one k_retrieve_slices workgroup per (group of kRetrieveQ queries, work item); a work item is a slice
// (set, first descriptor, count) of one set, at most slice_len descriptors, never across a set boundary.  An empty or
// skipped set has no item.  slice_len is kRetrieveSlice, doubled until the slice partials (8 bytes per item and query)
// number at most kRetrieveMaxPartials; at 2^16 = kRetrieveMaxSet every set is one slice and the partials are at most
// S nq <= 2^23, so the doubling ends.
#ifndef SG_RETRIEVE_PLAN_H_
#define SG_RETRIEVE_PLAN_H_

#include <cstdint>
#include <vector>

#include "slamgpu.h"

namespace sg {

constexpr int kRetrieveQ = 256;               // queries per workgroup of k_retrieve_slices (hamming.hip's kHmQ)
constexpr int kRetrieveTile = 128;            // descriptors per LDS tile (hamming.hip's kHmTile)
constexpr int kRetrieveSlice = 1024;          // descriptors per work item: a whole number of tiles
constexpr int kRetrieveMaxSet = 1 << 16;      // descriptors in one set
constexpr int kRetrieveMaxSets = 4096;
constexpr int64_t kRetrieveMaxDescriptors = (int64_t)1 << 22;   // in the database: 128 MiB
constexpr int kRetrieveMaxQuery = 1 << 20;
constexpr int64_t kRetrieveMaxCells = (int64_t)1 << 23;         // S * nq of one query
constexpr int64_t kRetrieveMaxPartials = (int64_t)1 << 24;      // work items * nq of one query
constexpr int kRetrieveClaimShift = 22;       // the claim key: (best_dist << 22) | query index
constexpr int64_t kRetrieveMinCapacity = 4096;                  // descriptors: the first device allocation
static_assert(kRetrieveSlice % kRetrieveTile == 0, "a slice is whole tiles");
static_assert(kRetrieveMaxQuery <= (1 << kRetrieveClaimShift), "the query index fits the claim key");
static_assert(kRetrieveMaxSet <= (1 << 22), "the index within a set fits the packed distance key");

// The sets of the database: set s holds descriptors offset[s] .. offset[s + 1] of the device buffer.
struct RetrieveDb {
  std::vector<int32_t> offset{0};   // [S + 1]
  int32_t sets() const { return (int32_t)offset.size() - 1; }
  int32_t size(int32_t s) const { return offset[s + 1] - offset[s]; }
  int32_t total() const { return offset.back(); }
};

// sg_matcher_db_add's argument check and bookkeeping: throws sg::Error(SG_EINVAL) and leaves db as it is, or appends
// the set and returns its number.
int32_t DbAppend(RetrieveDb* db, const uint64_t* desc, int32_t n);
// Capacity (descriptors) of the device buffer that holds `need` descriptors when it now holds `cap`: cap when that is
// enough, else at least double, at least kRetrieveMinCapacity, never above kRetrieveMaxDescriptors.
int64_t DbCapacity(int64_t cap, int64_t need);

struct RetrieveItem {
  int32_t set;     // the set
  int32_t first;   // first descriptor of the slice, an index within the set
  int32_t count;   // 1 .. slice_len
  int32_t base;    // offset[set] + first: the slice's first row of the device buffer
};
static_assert(sizeof(RetrieveItem) == 16, "read by the kernels as 4 ints");

struct RetrieveSet {
  int32_t item0;    // the set's first work item
  int32_t nitems;   // 0: empty or skipped
  int32_t offset;   // the set's first row of the device buffer (and of the claim array)
  int32_t n;        // its descriptors
};
static_assert(sizeof(RetrieveSet) == 16, "read by the kernels as 4 ints");

struct RetrievePlan {
  int32_t S = 0, nq = 0;
  int32_t slice_len = kRetrieveSlice;
  int32_t qgroups = 0;               // ceil(nq / kRetrieveQ): k_retrieve_slices runs qgroups x items.size() workgroups,
                                     // the merge and resolve kernels qgroups x S workgroups of kRetrieveQ threads
  std::vector<RetrieveSet> sets;     // [S]
  std::vector<RetrieveItem> items;   // sets in order, slices in order
  bool launch = false;               // nq > 0 and at least one item
};

// Every SG_EINVAL case of sg_matcher_db_query's contract (the handle is the caller's), then the plan.
void PlanQuery(const RetrieveDb& db, const uint64_t* query, int32_t nq, const sg_retrieve_options* o,
               const uint8_t* skip, const int32_t* score, int32_t k, const int32_t* top_set, const int32_t* top_score,
               RetrievePlan* out);

// Rule 5: the sets with score >= min_score that are not skipped, by (score descending, set ascending); the first k of
// them into top_set / top_score, the rest -1.
void RankSets(const int32_t* score, const uint8_t* skip, int32_t S, int32_t min_score, int32_t k, int32_t* top_set,
              int32_t* top_score);

// Rules 1-4 on the CPU for one set: per query the matched descriptor (an index within the set) and its distance, or
// -1, -1; returns the score.  desc: the set's n descriptors.
int32_t RetrieveSetCpu(const uint64_t* desc, int32_t n, const uint64_t* query, int32_t nq,
                       const sg_retrieve_options& o, int32_t* match, int32_t* match_dist);

// The whole contract on the CPU (rules 1-6), the argument checks included: what sg_matcher_db_query computes, from the
// database's descriptors on the host.
void RetrieveCpu(const RetrieveDb& db, const uint64_t* desc, const uint64_t* query, int32_t nq,
                 const sg_retrieve_options* o, const uint8_t* skip, int32_t* score, int32_t k, int32_t* top_set,
                 int32_t* top_score, int32_t* match, int32_t* match_dist);

}  // namespace sg

#endif  // SG_RETRIEVE_PLAN_H_
