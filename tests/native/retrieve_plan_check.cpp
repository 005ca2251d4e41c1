// CPU check of csrc/retrieve_plan.cpp, the host-only side of the keyframe descriptor database (sg_matcher_db_*): the
// database bookkeeping and its caps, the capacity rule, the slice work lists against brute force (no slice crosses a
// set, the slices cover every descriptor of every non-skipped set exactly once, nothing else is covered), the slice
// length rule and the launch shapes, the ranking, the CPU executor against a second brute-force restatement of rules
// 1-6, every SG_EINVAL case and the empty shapes.  Prints the constants that tests/retrieve_cases.py restates.  Built
// under AddressSanitizer and UBSan by tests/test_retrieve_plan.py.  No GPU, no HIP.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "common.h"
#include "retrieve_plan.h"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      if (++g_fail <= 20) {                              \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                        \
        std::printf("\n");                               \
      }                                                  \
    }                                                    \
  } while (0)

struct Lcg {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  uint64_t word() { return ((uint64_t)next() << 33) ^ ((uint64_t)next() << 11) ^ next(); }
};

sg_retrieve_options defaults() {
  sg_retrieve_options o{};
  o.max_dist = 64;
  o.ratio_percent = 80;
  o.min_score = 1;
  return o;
}

const uint64_t kDummy[4] = {0, 0, 0, 0};   // a non-null descriptor pointer where nothing is read

sg::RetrieveDb make_db(const std::vector<int32_t>& sizes) {
  sg::RetrieveDb db;
  for (int32_t n : sizes) sg::DbAppend(&db, kDummy, n);
  return db;
}

int append_code(sg::RetrieveDb* db, const uint64_t* desc, int32_t n) {
  try {
    sg::DbAppend(db, desc, n);
  } catch (const sg::Error& e) {
    return e.code;
  }
  return SG_OK;
}

struct Outs {
  std::vector<int32_t> score, top_set, top_score;
  Outs(int S, int k) : score((size_t)S + 1, 7), top_set((size_t)k + 1, 7), top_score((size_t)k + 1, 7) {}
  bool untouched() const {
    auto all7 = [](const std::vector<int32_t>& v) { return std::all_of(v.begin(), v.end(), [](int32_t x) { return x == 7; }); };
    return all7(score) && all7(top_set) && all7(top_score);
  }
};

int plan_code(const sg::RetrieveDb& db, const uint64_t* q, int32_t nq, const sg_retrieve_options* o,
              const uint8_t* skip, int32_t* score, int32_t k, int32_t* ts, int32_t* tsc,
              sg::RetrievePlan* keep = nullptr) {
  sg::RetrievePlan plan;
  try {
    sg::PlanQuery(db, q, nq, o, skip, score, k, ts, tsc, &plan);
  } catch (const sg::Error& e) {
    return e.code;
  }
  if (keep) *keep = plan;
  return SG_OK;
}

// ---------------------------------------------------------------------------------------------- bookkeeping
void check_bookkeeping() {
  sg::RetrieveDb db;
  CHECK(db.sets() == 0 && db.total() == 0, "a fresh database is empty");
  CHECK(sg::DbAppend(&db, kDummy, 5) == 0 && sg::DbAppend(&db, nullptr, 0) == 1 && sg::DbAppend(&db, kDummy, 3) == 2,
        "set numbers");
  CHECK(db.sets() == 3 && db.total() == 8 && db.size(0) == 5 && db.size(1) == 0 && db.size(2) == 3, "sizes");
  CHECK(db.offset == (std::vector<int32_t>{0, 5, 5, 8}), "offsets");
  const sg::RetrieveDb before = db;
  CHECK(append_code(nullptr, kDummy, 1) == SG_EINVAL, "null database");
  CHECK(append_code(&db, kDummy, -1) == SG_EINVAL, "negative n");
  CHECK(append_code(&db, nullptr, 1) == SG_EINVAL, "null descriptors");
  CHECK(append_code(&db, kDummy, sg::kRetrieveMaxSet + 1) == SG_EINVAL, "oversize set");
  CHECK(db.offset == before.offset, "a refused add changes nothing");
  CHECK(append_code(&db, kDummy, sg::kRetrieveMaxSet) == SG_OK, "a set of 65536");
  // 4096 sets, then one more
  sg::RetrieveDb many;
  for (int s = 0; s < sg::kRetrieveMaxSets; ++s) CHECK(append_code(&many, kDummy, s % 3) == SG_OK, "set %d", s);
  CHECK(append_code(&many, kDummy, 1) == SG_EINVAL && append_code(&many, nullptr, 0) == SG_EINVAL, "4097th set");
  CHECK(many.sets() == sg::kRetrieveMaxSets, "still 4096");
  // 2^22 descriptors, then one more
  sg::RetrieveDb full;
  for (int s = 0; s < 64; ++s) CHECK(append_code(&full, kDummy, sg::kRetrieveMaxSet) == SG_OK, "full set %d", s);
  CHECK(full.total() == sg::kRetrieveMaxDescriptors, "2^22 descriptors");
  CHECK(append_code(&full, kDummy, 1) == SG_EINVAL && append_code(&full, nullptr, 0) == SG_OK, "2^22 + 1 descriptors");
  // capacity: enough, at least doubling, a floor, the cap
  int64_t cap = 0, allocs = 0;
  for (int64_t need = 1; need <= sg::kRetrieveMaxDescriptors; need += 1 + need / 3) {
    const int64_t c = sg::DbCapacity(cap, need);
    CHECK(c >= need && c >= cap && c <= sg::kRetrieveMaxDescriptors, "capacity %lld for %lld", (long long)c, (long long)need);
    if (c != cap) {
      CHECK(c >= std::min<int64_t>(2 * cap, sg::kRetrieveMaxDescriptors) && c >= sg::kRetrieveMinCapacity, "geometric");
      ++allocs;
    }
    cap = c;
  }
  CHECK(allocs <= 12, "%lld allocations up to 2^22 descriptors", (long long)allocs);
  CHECK(sg::DbCapacity(4096, 4096) == 4096 && sg::DbCapacity(4096, 4097) == 8192 && sg::DbCapacity(0, 1) == 4096 &&
            sg::DbCapacity(4096, 20000) == 20000 && sg::DbCapacity(3000000, 3000001) == sg::kRetrieveMaxDescriptors,
        "capacity values");
}

// ---------------------------------------------------------------------------------------------- work lists
void check_plan(const std::vector<int32_t>& sizes, const std::vector<uint8_t>& skipv, int32_t nq, const char* what) {
  const sg::RetrieveDb db = make_db(sizes);
  const int S = db.sets();
  const uint8_t* skip = skipv.empty() ? nullptr : skipv.data();
  sg_retrieve_options o = defaults();
  Outs out(S, 2);
  sg::RetrievePlan p;
  const int rc = plan_code(db, kDummy, nq, &o, skip, out.score.data(), 2, out.top_set.data(), out.top_score.data(), &p);
  CHECK(rc == SG_OK, "%s: plan failed", what);
  if (rc != SG_OK) return;
  CHECK(out.untouched(), "%s: the planner writes no output", what);
  CHECK(p.S == S && p.nq == nq && p.qgroups == (nq + sg::kRetrieveQ - 1) / sg::kRetrieveQ, "%s: shapes", what);
  CHECK((int)p.sets.size() == S, "%s: set records", what);
  // the slice length: kRetrieveSlice doubled as little as the partial bound asks, never past one slice per set
  const int L = p.slice_len;
  auto items_at = [&](int len) {
    int64_t n = 0;
    for (int s = 0; s < S; ++s)
      if (!(skip && skip[s])) n += (sizes[(size_t)s] + len - 1) / len;
    return n;
  };
  CHECK(L >= sg::kRetrieveSlice && L <= sg::kRetrieveMaxSet && (L & (L - 1)) == 0, "%s: slice_len %d", what, L);
  CHECK(items_at(L) * nq <= sg::kRetrieveMaxPartials, "%s: %lld partials", what, (long long)(items_at(L) * nq));
  CHECK(L == sg::kRetrieveSlice || items_at(L / 2) * nq > sg::kRetrieveMaxPartials, "%s: slice_len doubled too far", what);
  CHECK((int64_t)p.items.size() == items_at(L), "%s: item count", what);
  // coverage by brute force: one counter per descriptor of the database
  std::vector<int> cover((size_t)db.total(), 0);
  int prev_set = -1, prev_end = 0;
  for (size_t w = 0; w < p.items.size(); ++w) {
    const sg::RetrieveItem& it = p.items[w];
    CHECK(it.set >= 0 && it.set < S, "%s: item set", what);
    if (it.set < 0 || it.set >= S) return;
    const int n = sizes[(size_t)it.set];
    CHECK(it.count >= 1 && it.count <= L && it.first >= 0 && it.first + it.count <= n, "%s: item %zu leaves its set", what, w);
    CHECK(it.base == db.offset[(size_t)it.set] + it.first, "%s: item base", what);
    CHECK(it.first % L == 0 && (it.count == L || it.first + it.count == n), "%s: only a set's last slice is short", what);
    CHECK(it.set > prev_set || (it.set == prev_set && it.first == prev_end), "%s: items in set and slice order", what);
    CHECK(it.set != prev_set ? it.first == 0 : true, "%s: a set's first slice starts at 0", what);
    prev_set = it.set;
    prev_end = it.first + it.count;
    const sg::RetrieveSet& r = p.sets[(size_t)it.set];
    CHECK((int)w >= r.item0 && (int)w < r.item0 + r.nitems, "%s: item outside its set's range", what);
    if (it.first >= 0 && it.first + it.count <= n)
      for (int j = 0; j < it.count; ++j) ++cover[(size_t)(it.base + j)];
  }
  for (int s = 0; s < S; ++s) {
    const bool skipped = skip && skip[s];
    const sg::RetrieveSet& r = p.sets[(size_t)s];
    CHECK(r.offset == db.offset[(size_t)s] && r.n == sizes[(size_t)s], "%s: set record %d", what, s);
    CHECK(r.nitems == (skipped ? 0 : (sizes[(size_t)s] + L - 1) / L), "%s: set %d has %d items", what, s, r.nitems);
    CHECK(r.item0 >= 0 && r.item0 + r.nitems <= (int)p.items.size(), "%s: set %d item range", what, s);
    for (int j = 0; j < sizes[(size_t)s]; ++j)
      CHECK(cover[(size_t)(db.offset[(size_t)s] + j)] == (skipped ? 0 : 1), "%s: descriptor %d of set %d covered %d times",
            what, j, s, cover[(size_t)(db.offset[(size_t)s] + j)]);
  }
  CHECK(p.launch == (nq > 0 && !p.items.empty()), "%s: launch", what);
}

void check_plans() {
  const int L = sg::kRetrieveSlice, T = sg::kRetrieveTile;
  check_plan({0, 1, 2, T - 1, T, T + 1, L, L + 1, 2 * L + 77}, {}, 600, "sizes");
  check_plan({0, 1, 2, T - 1, T, T + 1, L, L + 1, 2 * L + 77}, {0, 1, 0, 0, 1, 0, 0, 1, 0}, 257, "sizes, skips");
  check_plan({0, 1, 2, T - 1, T, T + 1, L, L + 1, 2 * L + 77}, {1, 1, 1, 1, 1, 1, 1, 1, 1}, 5, "all skipped");
  check_plan({0, 0, 0}, {}, 9, "only empty sets");
  check_plan({}, {}, 9, "no sets");
  check_plan({5, 6}, {}, 0, "no query");
  check_plan({sg::kRetrieveMaxSet, 1, sg::kRetrieveMaxSet}, {}, 1, "two full sets");
  // the partial bound: 64 full sets, queries that make the slice length double
  std::vector<int32_t> full(64, sg::kRetrieveMaxSet);
  check_plan(full, {}, 4096, "64 full sets, 4096 queries");          // 4096 items * 4096 = 2^24: no doubling
  check_plan(full, {}, 4097, "64 full sets, 4097 queries");          // one doubling
  check_plan(full, {}, 1 << 17, "64 full sets, 2^17 queries");       // S nq = 2^23: slices of 32768
  check_plan({sg::kRetrieveMaxSet, 3 * L, 7}, {}, sg::kRetrieveMaxQuery, "2^20 queries");   // slices of 8192
  Lcg r{77};
  for (int rep = 0; rep < 60; ++rep) {
    std::vector<int32_t> sizes(1 + r.next() % 40);
    std::vector<uint8_t> skip;
    for (int32_t& n : sizes) n = r.next() % 4 == 0 ? (int)(r.next() % 3) : (int)(r.next() % (3 * L + 50));
    if (rep % 2)
      for (size_t s = 0; s < sizes.size(); ++s) skip.push_back((uint8_t)(r.next() % 3 == 0 ? 1 + r.next() % 200 : 0));
    check_plan(sizes, skip, (int)(r.next() % 3000), "generated");
  }
}

// ---------------------------------------------------------------------------------------------- ranking
void check_ranking() {
  Lcg r{5};
  for (int rep = 0; rep < 200; ++rep) {
    const int S = (int)(r.next() % 12), k = (int)(r.next() % 15), min_score = (int)(r.next() % 4);
    std::vector<int32_t> score((size_t)S), ts((size_t)k + 1, 7), tsc((size_t)k + 1, 7);
    std::vector<uint8_t> skip((size_t)S);
    for (int s = 0; s < S; ++s) {
      skip[(size_t)s] = r.next() % 4 == 0;
      score[(size_t)s] = skip[(size_t)s] ? -1 : (int)(r.next() % 5);   // many equal scores
    }
    const bool with_skip = rep % 3 != 0;
    if (!with_skip)
      for (int s = 0; s < S; ++s)
        if (skip[(size_t)s]) score[(size_t)s] = 0;
    sg::RankSets(score.data(), with_skip ? skip.data() : nullptr, S, min_score, k, ts.data(), tsc.data());
    // brute force: pick the best remaining set k times
    std::vector<char> used((size_t)S, 0);
    for (int rk = 0; rk < k; ++rk) {
      int best = -1;
      for (int s = 0; s < S; ++s) {
        if (used[(size_t)s] || (with_skip && skip[(size_t)s]) || score[(size_t)s] < min_score) continue;
        if (best < 0 || score[(size_t)s] > score[(size_t)best]) best = s;   // s ascends: ties keep the lower index
      }
      if (best >= 0) used[(size_t)best] = 1;
      CHECK(ts[(size_t)rk] == best && tsc[(size_t)rk] == (best < 0 ? -1 : score[(size_t)best]), "rank %d of rep %d", rk, rep);
    }
    CHECK(ts[(size_t)k] == 7 && tsc[(size_t)k] == 7, "ranking writes k entries");
  }
}

// ---------------------------------------------------------------------------------------------- the executor
int popcount256(const uint64_t* a, const uint64_t* b) {
  int d = 0;
  for (int w = 0; w < 4; ++w)
    for (uint64_t x = a[w] ^ b[w]; x; x &= x - 1) ++d;
  return d;
}

// Rules 1-4 restated from the descriptor's side: all distances first, then per query its best and second, then per
// descriptor the claimant it keeps.
int brute_set(const uint64_t* t, int n, const uint64_t* q, int nq, const sg_retrieve_options& o,
              std::vector<int32_t>* match, std::vector<int32_t>* dist) {
  match->assign((size_t)nq, -1);
  dist->assign((size_t)nq, -1);
  if (n == 0) return 0;
  std::vector<int> d((size_t)nq * n), best((size_t)nq), cand((size_t)nq, 0);
  for (int i = 0; i < nq; ++i)
    for (int j = 0; j < n; ++j) d[(size_t)i * n + j] = popcount256(q + 4 * (size_t)i, t + 4 * (size_t)j);
  for (int i = 0; i < nq; ++i) {
    std::vector<int> row(d.begin() + (size_t)i * n, d.begin() + (size_t)(i + 1) * n);
    best[(size_t)i] = (int)(std::min_element(row.begin(), row.end()) - row.begin());   // the first minimum
    std::sort(row.begin(), row.end());
    const int bd = row[0], sd = n >= 2 ? row[1] : -1;
    cand[(size_t)i] = bd <= o.max_dist && (sd < 0 || 100 * bd <= o.ratio_percent * sd);
  }
  int score = 0;
  for (int j = 0; j < n; ++j) {
    int keep = -1;
    for (int i = 0; i < nq; ++i)
      if (cand[(size_t)i] && best[(size_t)i] == j && (keep < 0 || d[(size_t)i * n + j] < d[(size_t)keep * n + j])) keep = i;
    if (keep >= 0) {
      (*match)[(size_t)keep] = j;
      (*dist)[(size_t)keep] = d[(size_t)keep * n + j];
      ++score;
    }
  }
  return score;
}

void check_executor() {
  Lcg r{909};
  for (int rep = 0; rep < 40; ++rep) {
    const int S = 1 + (int)(r.next() % 6), nq = (int)(r.next() % 50), k = (int)(r.next() % 8);
    sg::RetrieveDb db;
    std::vector<uint64_t> desc;
    std::vector<int32_t> sizes;
    for (int s = 0; s < S; ++s) {
      const int n = r.next() % 5 == 0 ? (int)(r.next() % 3) : (int)(1 + r.next() % 40);
      sizes.push_back(n);
      for (int j = 0; j < n; ++j)
        for (int w = 0; w < 4; ++w) {
          // duplicates of an earlier row of the database: ties at zero and above
          const bool dup = !desc.empty() && desc.size() >= 8 && r.next() % 6 == 0 && w == 0;
          if (dup) {
            const size_t src = 4 * (r.next() % (desc.size() / 4));
            for (int v = 0; v < 4; ++v) desc.push_back(desc[src + v]);
            break;
          }
          desc.push_back(r.word());
        }
      sg::DbAppend(&db, kDummy, n);
    }
    CHECK((int64_t)desc.size() == 4 * (int64_t)db.total(), "generated database");
    // queries: rows of the database with 0..90 bits flipped (both sides of max_dist and of the ratio), and random rows
    std::vector<uint64_t> q((size_t)4 * nq);
    for (int i = 0; i < nq; ++i) {
      if (db.total() > 0 && r.next() % 5 != 0) {
        const size_t src = 4 * (r.next() % db.total());
        for (int w = 0; w < 4; ++w) q[(size_t)4 * i + w] = desc[src + w];
        const int flips = (int)(r.next() % (r.next() % 3 ? 12 : 91));
        for (int f = 0; f < flips; ++f) {
          const int b = (int)(r.next() % 256);
          q[(size_t)4 * i + (b >> 6)] ^= (uint64_t)1 << (b & 63);
        }
      } else {
        for (int w = 0; w < 4; ++w) q[(size_t)4 * i + w] = r.word();
      }
    }
    sg_retrieve_options o = defaults();
    if (rep % 4 == 1) o = sg_retrieve_options{256, 100, 0};
    if (rep % 4 == 2) o = sg_retrieve_options{(int32_t)(r.next() % 100), (int32_t)(1 + r.next() % 100), (int32_t)(r.next() % 3)};
    std::vector<uint8_t> skip;
    if (rep % 3 == 0)
      for (int s = 0; s < S; ++s) skip.push_back(r.next() % 3 == 0);
    const uint8_t* sk = skip.empty() ? nullptr : skip.data();
    std::vector<int32_t> score((size_t)S, 7), ts((size_t)k, 7), tsc((size_t)k, 7), match((size_t)k * nq, 7), md((size_t)k * nq, 7);
    const uint64_t* qp = nq ? q.data() : nullptr;
    sg::RetrieveCpu(db, desc.data(), qp, nq, &o, sk, score.data(), k, ts.data(), tsc.data(), match.data(), md.data());
    // the second statement
    std::vector<std::vector<int32_t>> bm((size_t)S), bdist((size_t)S);
    std::vector<int32_t> bscore((size_t)S);
    for (int s = 0; s < S; ++s) {
      if (sk && sk[s]) {
        bscore[(size_t)s] = -1;
        continue;
      }
      bscore[(size_t)s] = brute_set(desc.data() + 4 * (size_t)db.offset[(size_t)s], sizes[(size_t)s], q.data(), nq, o,
                                    &bm[(size_t)s], &bdist[(size_t)s]);
    }
    CHECK(score == bscore, "rep %d: scores", rep);
    std::vector<char> used((size_t)S, 0);
    for (int rk = 0; rk < k; ++rk) {
      int best = -1;
      for (int s = 0; s < S; ++s)
        if (!used[(size_t)s] && !(sk && sk[s]) && bscore[(size_t)s] >= o.min_score && (best < 0 || bscore[(size_t)s] > bscore[(size_t)best]))
          best = s;
      if (best >= 0) used[(size_t)best] = 1;
      CHECK(ts[(size_t)rk] == best && tsc[(size_t)rk] == (best < 0 ? -1 : bscore[(size_t)best]), "rep %d: rank %d", rep, rk);
      for (int i = 0; i < nq; ++i) {
        const int32_t em = best < 0 ? -1 : bm[(size_t)best][(size_t)i], ed = best < 0 ? -1 : bdist[(size_t)best][(size_t)i];
        CHECK(match[(size_t)rk * nq + i] == em && md[(size_t)rk * nq + i] == ed, "rep %d: rank %d query %d", rep, rk, i);
      }
    }
    // match and match_dist may be null
    std::vector<int32_t> score2((size_t)S, 7);
    sg::RetrieveCpu(db, desc.data(), qp, nq, &o, sk, score2.data(), k, ts.data(), tsc.data(), nullptr, nullptr);
    CHECK(score2 == score, "rep %d: null match rows", rep);
  }
}

// ---------------------------------------------------------------------------------------------- arguments
void check_arguments() {
  const sg::RetrieveDb db = make_db({5, 0, 9});
  sg_retrieve_options o = defaults();
  Outs out(3, 2);
  int32_t *sc = out.score.data(), *ts = out.top_set.data(), *tsc = out.top_score.data();
  CHECK(plan_code(db, kDummy, 1, &o, nullptr, sc, 2, ts, tsc) == SG_OK, "a good call");
  CHECK(plan_code(db, kDummy, 1, nullptr, nullptr, sc, 2, ts, tsc) == SG_EINVAL, "null options");
  CHECK(plan_code(db, kDummy, 1, &o, nullptr, nullptr, 2, ts, tsc) == SG_EINVAL, "null score with S > 0");
  CHECK(plan_code(sg::RetrieveDb{}, kDummy, 1, &o, nullptr, nullptr, 2, ts, tsc) == SG_OK, "null score with S == 0");
  CHECK(plan_code(db, kDummy, -1, &o, nullptr, sc, 2, ts, tsc) == SG_EINVAL, "nq < 0");
  CHECK(plan_code(db, nullptr, 1, &o, nullptr, sc, 2, ts, tsc) == SG_EINVAL, "null query with nq > 0");
  CHECK(plan_code(db, nullptr, 0, &o, nullptr, sc, 2, ts, tsc) == SG_OK, "null query with nq == 0");
  CHECK(plan_code(db, kDummy, 1, &o, nullptr, sc, -1, ts, tsc) == SG_EINVAL, "k < 0");
  CHECK(plan_code(db, kDummy, 1, &o, nullptr, sc, 2, nullptr, tsc) == SG_EINVAL, "null top_set with k > 0");
  CHECK(plan_code(db, kDummy, 1, &o, nullptr, sc, 2, ts, nullptr) == SG_EINVAL, "null top_score with k > 0");
  CHECK(plan_code(db, kDummy, 1, &o, nullptr, sc, 0, nullptr, nullptr) == SG_OK, "k == 0 needs no ranks");
  const int bad[][3] = {{-1, 80, 1}, {257, 80, 1}, {64, 0, 1}, {64, 101, 1}, {64, 80, -1}};
  for (const auto& b : bad) {
    sg_retrieve_options x{b[0], b[1], b[2]};
    CHECK(plan_code(db, kDummy, 1, &x, nullptr, sc, 2, ts, tsc) == SG_EINVAL, "options %d %d %d", b[0], b[1], b[2]);
    CHECK(plan_code(db, nullptr, 0, &x, nullptr, sc, 2, ts, tsc) == SG_EINVAL, "options %d %d %d with nq == 0", b[0], b[1], b[2]);
  }
  const int good[][3] = {{0, 1, 0}, {256, 100, 1 << 30}};
  for (const auto& g : good) {
    sg_retrieve_options x{g[0], g[1], g[2]};
    CHECK(plan_code(db, kDummy, 1, &x, nullptr, sc, 2, ts, tsc) == SG_OK, "options %d %d %d", g[0], g[1], g[2]);
  }
  // the caps of a query: nq <= 2^20 (the query is not read by the planner), S nq <= 2^23
  CHECK(plan_code(make_db({4}), kDummy, sg::kRetrieveMaxQuery, &o, nullptr, sc, 2, ts, tsc) == SG_OK, "2^20 queries");
  CHECK(plan_code(make_db({4}), kDummy, sg::kRetrieveMaxQuery + 1, &o, nullptr, sc, 2, ts, tsc) == SG_EINVAL, "2^20 + 1 queries");
  std::vector<int32_t> sixteen(16, 3), big_score(17, 7);
  CHECK(plan_code(make_db(sixteen), kDummy, 1 << 19, &o, nullptr, big_score.data(), 2, ts, tsc) == SG_OK, "S nq == 2^23");
  CHECK(plan_code(make_db(sixteen), kDummy, (1 << 19) + 1, &o, nullptr, big_score.data(), 2, ts, tsc) == SG_EINVAL, "S nq > 2^23");
  std::vector<uint8_t> all_skipped(16, 1);
  CHECK(plan_code(make_db(sixteen), kDummy, (1 << 19) + 1, &o, all_skipped.data(), big_score.data(), 2, ts, tsc) == SG_EINVAL,
        "S nq > 2^23 counts skipped sets too");
  CHECK(out.untouched() && std::all_of(big_score.begin(), big_score.end(), [](int32_t x) { return x == 7; }),
        "the planner writes no output");
  // the executor refuses the same calls, with nothing written
  int code = SG_OK;
  try {
    sg::RetrieveCpu(db, kDummy, kDummy, 1, nullptr, nullptr, sc, 2, ts, tsc, nullptr, nullptr);
  } catch (const sg::Error& e) {
    code = e.code;
  }
  CHECK(code == SG_EINVAL && out.untouched(), "the executor checks its arguments first");
}

void check_empty_shapes() {
  sg_retrieve_options o = defaults();
  // nq == 0: scores 0, -1 for skipped sets; nothing ranks with min_score 1, every unskipped set with min_score 0
  const sg::RetrieveDb db = make_db({5, 0, 9});
  std::vector<uint64_t> desc(4 * 14, 0x5555555555555555ull);
  const uint8_t skip[3] = {0, 0, 1};
  int32_t score[3] = {7, 7, 7}, ts[4] = {7, 7, 7, 7}, tsc[4] = {7, 7, 7, 7}, match[1] = {7};
  sg::RetrieveCpu(db, desc.data(), nullptr, 0, &o, skip, score, 3, ts, tsc, match, match);
  CHECK(score[0] == 0 && score[1] == 0 && score[2] == -1, "nq == 0: scores");
  CHECK(ts[0] == -1 && ts[1] == -1 && ts[2] == -1 && tsc[0] == -1 && tsc[2] == -1 && ts[3] == 7 && match[0] == 7, "nq == 0: ranks");
  o.min_score = 0;
  sg::RetrieveCpu(db, desc.data(), nullptr, 0, &o, skip, score, 3, ts, tsc, nullptr, nullptr);
  CHECK(ts[0] == 0 && ts[1] == 1 && ts[2] == -1 && tsc[0] == 0 && tsc[1] == 0 && tsc[2] == -1, "nq == 0, min_score 0");
  sg::RetrievePlan p;
  CHECK(plan_code(db, nullptr, 0, &o, skip, score, 3, ts, tsc, &p) == SG_OK && !p.launch && p.qgroups == 0 && p.items.size() == 1,
        "nq == 0: no launch");
  // S == 0
  const uint64_t q[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  int32_t m2[4] = {7, 7, 7, 7}, d2[4] = {7, 7, 7, 7};
  ts[0] = ts[1] = tsc[0] = tsc[1] = 7;
  sg::RetrieveCpu(sg::RetrieveDb{}, nullptr, q, 2, &o, nullptr, nullptr, 2, ts, tsc, m2, d2);
  CHECK(ts[0] == -1 && ts[1] == -1 && tsc[0] == -1 && tsc[1] == -1, "S == 0: ranks");
  CHECK(std::all_of(m2, m2 + 4, [](int32_t x) { return x == -1; }) && std::all_of(d2, d2 + 4, [](int32_t x) { return x == -1; }),
        "S == 0: rows");
  CHECK(plan_code(sg::RetrieveDb{}, q, 2, &o, nullptr, nullptr, 0, nullptr, nullptr, &p) == SG_OK && !p.launch && p.qgroups == 1,
        "S == 0: no launch");
}

}  // namespace

int main() {
  std::printf("kRetrieveQ %d kRetrieveTile %d kRetrieveSlice %d kRetrieveClaimShift %d\n", sg::kRetrieveQ, sg::kRetrieveTile,
              sg::kRetrieveSlice, sg::kRetrieveClaimShift);
  check_bookkeeping();
  check_plans();
  check_ranking();
  check_executor();
  check_arguments();
  check_empty_shapes();
  if (g_fail) {
    std::printf("retrieve_plan_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("retrieve_plan_check OK\n");
  return 0;
}
