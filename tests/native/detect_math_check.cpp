// detect_math_check.cpp — stand-alone CPU program over csrc/detect_math.h (tests/test_detect_math.py builds it with
// -fsanitize=address,undefined and compares its answers with the numpy reference).
//
//   detect_math_check <cases>
//
// <cases> is a binary file, little endian: int32 L; per level array: int32 pyramid level, int32 w, int32 h, then
// w * h float32 pixels; int32 R; per run: int32 depth, depth x int32 index of the level array of each pyramid level,
// int32 first_level, int32 num_levels (> 0), float32 t_lo, float32 t_hi, int32 border, int32 per_cell,
// int32 max_keypoints.  A run is what Tracker::Detect does with the kernel replaced by DetectLevelCells: the cell
// slots of the selected levels, then DetectCompact.  Printed per run: "run r count n", one line "k x y level
// scorebits" per keypoint (x, y level-0 pixels, the score's bits in hexadecimal), one line "l level width height
// cells candidates low_cells keypoints" per pyramid level.  Then the program's own checks of the ring table, the
// score and the key order on hand-made inputs.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "detect_math.h"

namespace {

struct Level {
  int level, w, h;
  std::vector<float> px;
};

template <typename T>
bool Get(FILE* f, T* v, size_t n = 1) {
  return fread(v, sizeof(T), n, f) == n;
}

int Fail(const char* what) {
  printf("detect_math_check FAILED: %s\n", what);
  return 1;
}

// d with `n` ring pixels from `start` at +v and the rest at rest
void Arc(float* d, int start, int n, float v, float rest) {
  for (int i = 0; i < 16; ++i) d[i] = rest;
  for (int j = 0; j < n; ++j) d[(start + j) & 15] = v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return Fail("usage: detect_math_check <cases>");
  FILE* f = fopen(argv[1], "rb");
  if (!f) return Fail("cannot open the cases");
  int32_t L = 0;
  if (!Get(f, &L) || L < 0 || L > 64) return Fail("bad level count");
  std::vector<Level> lv(L);
  for (auto& l : lv) {
    int32_t hdr[3];
    if (!Get(f, hdr, 3) || hdr[0] < 0 || hdr[0] > 7 || hdr[1] < 1 || hdr[2] < 1 || hdr[1] > 4096 || hdr[2] > 4096)
      return Fail("bad level header");
    l.level = hdr[0];
    l.w = hdr[1];
    l.h = hdr[2];
    l.px.resize((size_t)l.w * l.h);
    if (!Get(f, l.px.data(), l.px.size())) return Fail("short level");
  }
  int32_t R = 0;
  if (!Get(f, &R) || R < 0 || R > 4096) return Fail("bad run count");
  for (int r = 0; r < R; ++r) {
    int32_t depth = 0, idx[sg::kDetMaxDepth], first = 0, num = 0, ints[3];
    float t[2];
    if (!Get(f, &depth) || depth < 1 || depth > sg::kDetMaxDepth || !Get(f, idx, depth)) return Fail("bad run depth");
    if (!Get(f, &first) || !Get(f, &num) || !Get(f, t, 2) || !Get(f, ints, 3)) return Fail("short run");
    const int border = ints[0], per_cell = ints[1], max_keypoints = ints[2];
    if (first < 0 || num < 1 || first + num > depth || border < sg::kDetMinBorder || border > sg::kDetMaxBorder ||
        per_cell < 1 || per_cell > sg::kDetMaxPerCell || max_keypoints < 0 || !(t[0] >= 0.f) || !(t[0] <= t[1]))
      return Fail("bad run options");
    std::vector<sg_detect_level> per(depth);
    for (int l = 0; l < depth; ++l) {
      if (idx[l] < 0 || idx[l] >= L || lv[idx[l]].level != l) return Fail("bad level index");
      per[l] = sg_detect_level{lv[idx[l]].w, lv[idx[l]].h, 0, 0, 0, 0};
    }
    std::vector<sg::DetLevel> sel(num);
    int cells = 0;
    for (int i = 0; i < num; ++i) {
      const Level& l = lv[idx[first + i]];
      sel[i] = sg::DetLevel{first + i, l.w, l.h, cells, sg::DetectCells(l.w, l.h)};
      cells += sel[i].cells;
    }
    std::vector<uint64_t> slots((size_t)cells * per_cell, ~0ull);
    std::vector<sg::DetCellInfo> info(cells);
    for (int i = 0; i < num; ++i) {
      const Level& l = lv[idx[first + i]];
      sg::DetectLevelCells(l.px.data(), l.w, l.h, sg::DetectThreshold(t[0]), sg::DetectThreshold(t[1]), border,
                           per_cell, slots.data() + (size_t)sel[i].cell0 * per_cell, info.data() + sel[i].cell0);
    }
    const std::vector<sg::DetKeypoint> kp =
        sg::DetectCompact(sel, slots.data(), info.data(), per_cell, max_keypoints, per.data());
    printf("run %d count %zu\n", r, kp.size());
    for (const auto& k : kp)
      printf("k %d %d %d %08" PRIx32 "\n", (int)k.x, (int)k.y, (int)k.level, sg::DetectFloatBits(k.score));
    for (int l = 0; l < depth; ++l)
      printf("l %d %d %d %d %d %d %d\n", l, per[l].width, per[l].height, per[l].cells, per[l].candidates,
             per[l].low_cells, per[l].keypoints);
  }
  fclose(f);

  // the ring: 16 distinct offsets of the radius-3 circle, clockwise from the top (y down), each a king's move on
  const int ex[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
  const int ey[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
  for (int i = 0; i < 16; ++i) {
    const int x = sg::kDetRing.dx[i], y = sg::kDetRing.dy[i], nx = sg::kDetRing.dx[(i + 1) & 15],
              ny = sg::kDetRing.dy[(i + 1) & 15];
    if (x != ex[i] || y != ey[i]) return Fail("ring table");
    if (std::abs(nx - x) > 1 || std::abs(ny - y) > 1) return Fail("ring is not connected");
    if (x * ny - y * nx <= 0) return Fail("ring is not clockwise");
    if (sg::kDetRing.dx[(i + 8) & 15] != -x || sg::kDetRing.dy[(i + 8) & 15] != -y) return Fail("ring is not symmetric");
  }
  // the score: an arc of nine at +v over a rest of -1 scores v wherever it starts, an arc of eight does not; the dark
  // side likewise; the score is the arc's smallest member
  float d[16];
  for (int k = 0; k < 16; ++k) {
    Arc(d, k, 9, 0.5f, -1.f);
    if (sg::DetectScore(d) != 0.5f) return Fail("bright arc of nine");
    Arc(d, k, 8, 0.5f, -0.25f);
    if (sg::DetectScore(d) != -0.25f) return Fail("bright arc of eight");
    Arc(d, k, 9, -0.5f, 1.f);
    if (sg::DetectScore(d) != 0.5f) return Fail("dark arc of nine");
    Arc(d, k, 12, 0.75f, 0.f);
    d[(k + 5) & 15] = 0.125f;   // splits the twelve into five and six: no arc of nine is left above 0.125
    if (sg::DetectScore(d) != 0.125f) return Fail("split arc");
    Arc(d, k, 16, 0.75f, 0.f);
    d[k] = 0.25f;
    d[(k + 9) & 15] = 0.5f;     // every arc of nine holds one of the two; the arc k + 1 .. k + 9 only the 0.5
    if (sg::DetectScore(d) != 0.5f) return Fail("two low members");
  }
  for (int i = 0; i < 16; ++i) d[i] = 0.f;
  if (sg::DetectScore(d) != 0.f) return Fail("flat ring");
  // the quick reject never refuses a pixel whose score exceeds the threshold
  for (int k = 0; k < 16; ++k)
    for (int sign = -1; sign <= 1; sign += 2) {
      Arc(d, k, 9, sign * 0.5f, sign * -1.f);
      if (!sg::DetectMayExceed(d[0], d[4], d[8], d[12], 0.25f)) return Fail("quick reject refused a corner");
    }
  if (sg::DetectMayExceed(0.f, 0.f, 0.f, 0.f, 0.f) || sg::DetectMayExceed(0.5f, -0.5f, 0.5f, -0.5f, 0.25f))
    return Fail("quick reject let a flat ring or an alternating one through");
  // the suppression on a plateau: of equal neighbours the first in row-major order survives
  {
    const float s[25] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0};
    int survivors = 0;
    for (int y = 1; y < 4; ++y)
      for (int x = 1; x < 4; ++x) survivors += sg::DetectIsMax(s + 5 * y + x, 5) ? 100 + 5 * y + x : 0;
    if (survivors != 100 + 6) return Fail("plateau: exactly the first pixel survives");
  }
  // the key: score first, then the smaller index; it gives score and index back
  {
    const uint64_t a = sg::DetectKey(0.5f, 1000), b = sg::DetectKey(0.5f, 999), c = sg::DetectKey(0.25f, 0),
                   e = sg::DetectKey(1e-30f, 0x7FFFFFFF);
    if (!(b > a && a > c && c > e && e != 0)) return Fail("key order");
    if (sg::DetectKeyScore(a) != 0.5f || sg::DetectKeyIndex(a) != 1000 || sg::DetectKeyIndex(e) != 0x7FFFFFFF ||
        sg::DetectKeyIndex(c) != 0)
      return Fail("key round trip");
    if (sg::DetectEligible(c, true, 0.25f) || !sg::DetectEligible(c, false, 0.25f) || !sg::DetectEligible(a, true, 0.25f) ||
        sg::DetectEligible(0, false, 0.f))
      return Fail("eligibility");
    if (sg::DetectFloatBits(sg::DetectThreshold(-0.0f)) != 0) return Fail("threshold -0");
  }
  // the cap on hand-made slots: two levels, ties across levels go to the lower level, then to the smaller index
  {
    const std::vector<sg::DetLevel> two = {{0, 64, 32, 0, 2}, {1, 32, 16, 2, 1}};
    const uint64_t slots[6] = {sg::DetectKey(0.5f, 70), sg::DetectKey(0.25f, 5), sg::DetectKey(0.5f, 40), 0,
                               sg::DetectKey(0.5f, 3), sg::DetectKey(0.125f, 9)};
    const sg::DetCellInfo info[3] = {{7, 0}, {1, 1}, {4, 0}};
    sg_detect_level per[2] = {{64, 32, 0, 0, 0, 0}, {32, 16, 0, 0, 0, 0}};
    auto kp = sg::DetectCompact(two, slots, info, 2, 2, per);
    if (kp.size() != 2 || kp[0].x != 6.f || kp[0].y != 1.f || kp[1].x != 40.f || kp[1].y != 0.f || kp[1].level != 0)
      return Fail("cap: the two level-0 keypoints of score 0.5 stay, in output order");
    if (per[0].cells != 2 || per[0].candidates != 8 || per[0].low_cells != 1 || per[0].keypoints != 2 ||
        per[1].cells != 1 || per[1].candidates != 4 || per[1].keypoints != 0)
      return Fail("cap: per-level record");
    kp = sg::DetectCompact(two, slots, info, 2, 3, nullptr);
    if (kp.size() != 3 || kp[2].level != 1 || kp[2].x != 6.f || kp[2].y != 0.f) return Fail("cap of three");
    kp = sg::DetectCompact(two, slots, info, 2, 0, nullptr);
    if (kp.size() != 5 || kp[1].score != 0.25f || kp[4].score != 0.125f) return Fail("no cap");
  }
  printf("detect_math_check OK\n");
  return 0;
}
