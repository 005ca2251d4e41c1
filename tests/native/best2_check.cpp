// best2_check.cpp — stand-alone CPU program over csrc/best2.h, the packed-key best / second-best rule of the descriptor
// matchers (tests/test_best2_math.py builds it with -fsanitize=address,undefined and runs it).  Exhaustive over small
// inputs: the fold, the merge in every split and order, the tie rule, the 256-bit distance, the decode and the host's
// check of a result.  Prints the number of cases of each kind and "best2_check OK".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "best2.h"

namespace {

using sg::kBest2Inf;

struct U4 {
  uint32_t x, y, z, w;
};

int Fail(const char* what) {
  std::printf("best2_check FAILED: %s\n", what);
  return 1;
}

constexpr uint32_t Key(uint32_t dist, uint32_t index) { return (dist << sg::kBest2Shift) | index; }

// Seven distinct keys: equal distances with different indices, the extremes of both fields.
const uint32_t kPool[7] = {Key(0, 0),   Key(0, 5), Key(3, 1), Key(3, 2), Key(17, 4), Key(256, 0),
                           Key(256, sg::kBest2IndexMask)};

struct Pair {
  uint32_t m1 = kBest2Inf, m2 = kBest2Inf;
  bool operator==(const Pair& o) const { return m1 == o.m1 && m2 == o.m2; }
};

// (min, second min) of a set of distinct keys, by sorting.
Pair Sorted(std::vector<uint32_t> keys) {
  std::sort(keys.begin(), keys.end());
  Pair p;
  if (keys.size() > 0) p.m1 = keys[0];
  if (keys.size() > 1) p.m2 = keys[1];
  return p;
}

Pair Fold(const std::vector<uint32_t>& keys) {
  Pair p;
  for (uint32_t k : keys) sg::Best2Take(k, p.m1, p.m2);
  return p;
}

int Popcount256(const U4& a0, const U4& a1, const U4& b0, const U4& b1) {
  const uint32_t a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
  const uint32_t b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  int n = 0;
  for (int i = 0; i < 8; ++i)
    for (int bit = 0; bit < 32; ++bit) n += ((a[i] >> bit) & 1u) != ((b[i] >> bit) & 1u);
  return n;
}

bool SameResult(const sg::Best2Result& r, int32_t index, int32_t best, int32_t second, int32_t count) {
  return r.index == index && r.best == best && r.second == second && r.count == count;
}

}  // namespace

int main() {
  // 1. every sequence of up to 6 symbols, a symbol being one of the seven keys or the padding, with no key twice
  long folds = 0;
  for (int len = 0; len <= 6; ++len) {
    int total = 1;
    for (int i = 0; i < len; ++i) total *= 8;
    for (int code = 0; code < total; ++code) {
      std::vector<uint32_t> seq, set;
      unsigned used = 0;
      bool twice = false;
      for (int i = 0, c = code; i < len; ++i, c /= 8) {
        const int sym = c % 8;
        seq.push_back(sym == 7 ? kBest2Inf : kPool[sym]);
        if (sym == 7) continue;
        twice = twice || ((used >> sym) & 1u);
        used |= 1u << sym;
        set.push_back(kPool[sym]);
      }
      if (twice) continue;
      if (!(Fold(seq) == Sorted(set))) return Fail("the fold is not (min, second min) of the set");
      ++folds;
    }
  }
  {
    Pair none = Fold({}), one = Fold({kPool[2]});
    if (none.m1 != kBest2Inf || none.m2 != kBest2Inf) return Fail("the empty fold");
    if (one.m1 != kPool[2] || one.m2 != kBest2Inf) return Fail("the one-element fold");
  }

  // 2. every subset of up to 6 of the keys, every assignment of its keys to three parts (so every split into two or
  // three parts, empty parts included), the parts merged in every order
  long merges = 0;
  for (unsigned mask = 0; mask < (1u << 7); ++mask) {
    std::vector<uint32_t> set;
    for (int i = 0; i < 7; ++i)
      if ((mask >> i) & 1u) set.push_back(kPool[i]);
    if (set.size() > 6) continue;
    const Pair whole = Fold(set);
    int assignments = 1;
    for (size_t i = 0; i < set.size(); ++i) assignments *= 3;
    for (int code = 0; code < assignments; ++code) {
      std::vector<uint32_t> part[3];
      for (size_t i = 0, c = code; i < set.size(); ++i, c /= 3) part[c % 3].push_back(set[i]);
      const Pair res[3] = {Fold(part[0]), Fold(part[1]), Fold(part[2])};
      int order[3] = {0, 1, 2};
      do {
        Pair acc;   // as the slice merges start: nothing seen
        for (int o : order) sg::Best2Merge(acc.m1, acc.m2, res[o].m1, res[o].m2);
        if (!(acc == whole)) return Fail("a merge of the parts differs from the fold of the whole");
        Pair two = res[order[0]];   // and started from a part's own answer
        sg::Best2Merge(two.m1, two.m2, res[order[1]].m1, res[order[1]].m2);
        sg::Best2Merge(two.m1, two.m2, res[order[2]].m1, res[order[2]].m2);
        if (!(two == whole)) return Fail("a merge started from a part differs from the fold of the whole");
        ++merges;
      } while (std::next_permutation(order, order + 3));
    }
  }

  // 3. equal distances: the lower index wins, in either order
  for (int flip = 0; flip < 2; ++flip) {
    const uint32_t a = Key(9, 40), b = Key(9, 7);
    const Pair p = Fold(flip ? std::vector<uint32_t>{a, b} : std::vector<uint32_t>{b, a});
    const sg::Best2Result r = sg::Best2Decode(p.m1, p.m2, 2);
    if (!SameResult(r, 7, 9, 9, 2)) return Fail("a tie in distance does not go to the lower index");
  }

  // 4. the 256-bit distance against a bit-by-bit count
  long distances = 0;
  {
    const U4 zero{0, 0, 0, 0}, ones{~0u, ~0u, ~0u, ~0u};
    if (sg::Hamming256(zero, zero, zero, zero) != 0 || sg::Hamming256(ones, ones, ones, ones) != 0 ||
        sg::Hamming256(zero, zero, ones, ones) != 256 || sg::Hamming256(ones, zero, zero, zero) != 128)
      return Fail("Hamming256 of all-zero / all-one operands");
    for (int bit = 0; bit < 256; ++bit) {
      uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      w[bit / 32] = 1u << (bit % 32);
      const U4 s0{w[0], w[1], w[2], w[3]}, s1{w[4], w[5], w[6], w[7]};
      if (sg::Hamming256(s0, s1, zero, zero) != 1 || sg::Hamming256(ones, ones, s0, s1) != 255)
        return Fail("Hamming256 of a single-bit operand");
      ++distances;
    }
    std::mt19937 rng(20240607u);
    for (int i = 0; i < 2000; ++i) {
      U4 v[4];
      for (U4& u : v) u = U4{(uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng()};
      if (i % 4 == 1) v[2] = v[0];   // (shared halves: small distances too)
      if ((int)sg::Hamming256(v[0], v[1], v[2], v[3]) != Popcount256(v[0], v[1], v[2], v[3]))
        return Fail("Hamming256 differs from the bit-by-bit count");
      ++distances;
    }
  }

  // 5. the decode and the host's check on the boundary values
  {
    using sg::Best2Decode;
    using sg::Best2ResultOk;
    if (!SameResult(Best2Decode(kBest2Inf, kBest2Inf, 0), -1, -1, -1, 0)) return Fail("decode of no candidate");
    if (!SameResult(Best2Decode(Key(0, 3), kBest2Inf, 1), 3, 0, -1, 1)) return Fail("decode of one candidate");
    if (!SameResult(Best2Decode(Key(0, 3), Key(256, 4), 2), 3, 0, 256, 2)) return Fail("decode of two candidates");
    if (!SameResult(Best2Decode(Key(256, sg::kBest2IndexMask), Key(256, 0), 5), (int32_t)sg::kBest2IndexMask, 256, 256, 5))
      return Fail("decode of the largest key");
    // accepted: count 0, 1, 2; distances 0 and 256; second == best; the last index; the largest count
    const bool good = Best2ResultOk(-1, -1, -1, 0, 10, 10) && Best2ResultOk(-1, -1, -1, 0, 0, 0) &&
                      Best2ResultOk(3, 0, -1, 1, 10, 10) && Best2ResultOk(3, 256, -1, 1, 10, 10) &&
                      Best2ResultOk(3, 0, 256, 2, 10, 10) && Best2ResultOk(3, 0, 0, 2, 10, 10) &&
                      Best2ResultOk(3, 256, 256, 2, 10, 10) && Best2ResultOk(9, 7, 7, 10, 10, 10) &&
                      Best2ResultOk(0, 7, 8, 2, 1, 2);
    if (!good) return Fail("Best2ResultOk rejects a valid result");
    const bool bad = Best2ResultOk(-1, -1, -1, -1, 10, 10) ||   // count below 0
                     Best2ResultOk(3, 0, 5, 11, 10, 10) ||      // count above max_count
                     Best2ResultOk(3, 0, -1, 0, 10, 10) ||      // a best without a candidate
                     Best2ResultOk(-1, -1, -1, 1, 10, 10) ||    // a candidate without a best
                     Best2ResultOk(3, 0, 5, 1, 10, 10) ||       // a second with one candidate
                     Best2ResultOk(3, 0, -1, 2, 10, 10) ||      // two candidates without a second
                     Best2ResultOk(-2, -1, -1, 0, 10, 10) ||    // an index below -1
                     Best2ResultOk(-1, 0, -1, 0, 10, 10) ||     // no best, but a distance
                     Best2ResultOk(10, 0, -1, 1, 10, 10) ||     // index == max_index
                     Best2ResultOk(3, -1, -1, 1, 10, 10) ||     // a best without a distance
                     Best2ResultOk(3, 257, -1, 1, 10, 10) ||    // distance above 256
                     Best2ResultOk(3, 5, -2, 1, 10, 10) ||      // a second below -1
                     Best2ResultOk(3, 5, 4, 2, 10, 10) ||       // second below best
                     Best2ResultOk(3, 5, 257, 2, 10, 10);       // second above 256
    if (bad) return Fail("Best2ResultOk accepts an invalid result");
  }

  std::printf("folds %ld merges %ld distances %ld\n", folds, merges, distances);
  std::printf("best2_check OK\n");
  return 0;
}
