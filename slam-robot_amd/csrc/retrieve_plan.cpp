// retrieve_plan.cpp — see retrieve_plan.h.
#include "retrieve_plan.h"

#include <algorithm>
#include <numeric>

#include "common.h"

namespace sg {

int32_t DbAppend(RetrieveDb* db, const uint64_t* desc, int32_t n) {
  SG_REQUIRE(db, SG_EINVAL, "null database");
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative descriptor count");
  SG_REQUIRE(n == 0 || desc, SG_EINVAL, "null descriptors");
  SG_REQUIRE(n <= kRetrieveMaxSet, SG_EINVAL, "more than 65536 descriptors in one set");
  SG_REQUIRE(db->sets() < kRetrieveMaxSets, SG_EINVAL, "more than 4096 sets");
  SG_REQUIRE((int64_t)db->total() + n <= kRetrieveMaxDescriptors, SG_EINVAL, "more than 2^22 descriptors in all");
  db->offset.push_back(db->total() + n);
  return db->sets() - 1;
}

int64_t DbCapacity(int64_t cap, int64_t need) {
  if (need <= cap) return cap;
  return std::min(kRetrieveMaxDescriptors, std::max({need, 2 * cap, kRetrieveMinCapacity}));
}

namespace {

int64_t CountItems(const RetrieveDb& db, const uint8_t* skip, int32_t slice_len) {
  int64_t items = 0;
  for (int32_t s = 0; s < db.sets(); ++s)
    if (!(skip && skip[s])) items += (db.size(s) + slice_len - 1) / slice_len;
  return items;
}

}  // namespace

void PlanQuery(const RetrieveDb& db, const uint64_t* query, int32_t nq, const sg_retrieve_options* o,
               const uint8_t* skip, const int32_t* score, int32_t k, const int32_t* top_set, const int32_t* top_score,
               RetrievePlan* out) {
  SG_REQUIRE(o && out, SG_EINVAL, "null options");
  SG_REQUIRE(o->max_dist >= 0 && o->max_dist <= 256, SG_EINVAL, "max_dist must be in 0..256");
  SG_REQUIRE(o->ratio_percent >= 1 && o->ratio_percent <= 100, SG_EINVAL, "ratio_percent must be in 1..100");
  SG_REQUIRE(o->min_score >= 0, SG_EINVAL, "min_score must be >= 0");
  const int32_t S = db.sets();
  SG_REQUIRE(S == 0 || score, SG_EINVAL, "null score");
  SG_REQUIRE(nq >= 0, SG_EINVAL, "negative query count");
  SG_REQUIRE(nq == 0 || query, SG_EINVAL, "null query");
  SG_REQUIRE(k >= 0, SG_EINVAL, "negative k");
  SG_REQUIRE(k == 0 || (top_set && top_score), SG_EINVAL, "null top_set or top_score");
  SG_REQUIRE(nq <= kRetrieveMaxQuery, SG_EINVAL, "more than 2^20 query descriptors");
  SG_REQUIRE((int64_t)S * nq <= kRetrieveMaxCells, SG_EINVAL, "sets * nq is above 2^23: split the query");
  *out = RetrievePlan{};
  out->S = S;
  out->nq = nq;
  out->qgroups = (nq + kRetrieveQ - 1) / kRetrieveQ;
  out->sets.resize((size_t)S);
  int32_t L = kRetrieveSlice;
  while (L < kRetrieveMaxSet && CountItems(db, skip, L) * nq > kRetrieveMaxPartials) L *= 2;
  out->slice_len = L;
  for (int32_t s = 0; s < S; ++s) {
    const int32_t n = db.size(s);
    RetrieveSet& r = out->sets[(size_t)s];
    r.item0 = (int32_t)out->items.size();
    r.offset = db.offset[(size_t)s];
    r.n = n;
    if (!(skip && skip[s]))
      for (int32_t first = 0; first < n; first += L)
        out->items.push_back(RetrieveItem{s, first, std::min(L, n - first), r.offset + first});
    r.nitems = (int32_t)out->items.size() - r.item0;
  }
  out->launch = nq > 0 && !out->items.empty();
}

void RankSets(const int32_t* score, const uint8_t* skip, int32_t S, int32_t min_score, int32_t k, int32_t* top_set,
              int32_t* top_score) {
  std::vector<int32_t> order;
  for (int32_t s = 0; s < S; ++s)
    if (!(skip && skip[s]) && score[s] >= min_score) order.push_back(s);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return score[a] > score[b]; });
  for (int32_t r = 0; r < k; ++r) {
    const bool have = r < (int32_t)order.size();
    top_set[r] = have ? order[(size_t)r] : -1;
    top_score[r] = have ? score[order[(size_t)r]] : -1;
  }
}

int32_t RetrieveSetCpu(const uint64_t* desc, int32_t n, const uint64_t* query, int32_t nq,
                       const sg_retrieve_options& o, int32_t* match, int32_t* match_dist) {
  std::fill(match, match + nq, -1);
  std::fill(match_dist, match_dist + nq, -1);
  if (n == 0) return 0;
  std::vector<int32_t> owner((size_t)n, -1), owner_dist((size_t)n, 0);   // the claimant with the smallest (dist, i)
  std::vector<int32_t> bi((size_t)nq, -1), bd((size_t)nq, -1);
  for (int32_t i = 0; i < nq; ++i) {
    const uint64_t* q = query + 4 * (size_t)i;
    int32_t b = 1 << 30, bj = -1, sd = 1 << 30;
    for (int32_t j = 0; j < n; ++j) {
      const uint64_t* t = desc + 4 * (size_t)j;
      const int32_t d = __builtin_popcountll(q[0] ^ t[0]) + __builtin_popcountll(q[1] ^ t[1]) +
                        __builtin_popcountll(q[2] ^ t[2]) + __builtin_popcountll(q[3] ^ t[3]);
      if (d < b) {
        sd = b;
        b = d;
        bj = j;
      } else if (d < sd) {
        sd = d;
      }
    }
    const bool ratio_ok = n < 2 || 100 * b <= o.ratio_percent * sd;
    if (b > o.max_dist || !ratio_ok) continue;
    bi[(size_t)i] = bj;
    bd[(size_t)i] = b;
    if (owner[(size_t)bj] < 0 || b < owner_dist[(size_t)bj]) {   // i ascends: an equal distance keeps the earlier query
      owner[(size_t)bj] = i;
      owner_dist[(size_t)bj] = b;
    }
  }
  int32_t matched = 0;
  for (int32_t i = 0; i < nq; ++i)
    if (bi[(size_t)i] >= 0 && owner[(size_t)bi[(size_t)i]] == i) {
      match[i] = bi[(size_t)i];
      match_dist[i] = bd[(size_t)i];
      ++matched;
    }
  return matched;
}

void RetrieveCpu(const RetrieveDb& db, const uint64_t* desc, const uint64_t* query, int32_t nq,
                 const sg_retrieve_options* o, const uint8_t* skip, int32_t* score, int32_t k, int32_t* top_set,
                 int32_t* top_score, int32_t* match, int32_t* match_dist) {
  RetrievePlan plan;
  PlanQuery(db, query, nq, o, skip, score, k, top_set, top_score, &plan);
  const int32_t S = db.sets();
  SG_REQUIRE(db.total() == 0 || desc, SG_EINVAL, "null database descriptors");
  std::vector<int32_t> cm((size_t)S * nq, -1), cd((size_t)S * nq, -1);
  for (int32_t s = 0; s < S; ++s) {
    if (skip && skip[s]) {
      score[s] = -1;
      continue;
    }
    score[s] = RetrieveSetCpu(desc + 4 * (size_t)db.offset[(size_t)s], db.size(s), query, nq, *o,
                              cm.data() + (size_t)s * nq, cd.data() + (size_t)s * nq);
  }
  RankSets(score, skip, S, o->min_score, k, top_set, top_score);
  for (int32_t r = 0; r < k; ++r)
    for (int32_t i = 0; i < nq; ++i) {
      const int32_t s = top_set[r];
      if (match) match[(size_t)r * nq + i] = s >= 0 ? cm[(size_t)s * nq + i] : -1;
      if (match_dist) match_dist[(size_t)r * nq + i] = s >= 0 ? cd[(size_t)s * nq + i] : -1;
    }
}

}  // namespace sg
