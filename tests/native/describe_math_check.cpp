// describe_math_check.cpp — stand-alone CPU program over csrc/describe_math.h (tests/test_describe_math.py builds it
// with -fsanitize=address,undefined and compares its answers with the numpy reference).
//
//   describe_math_check <cases>
//
// <cases> is a binary file, little endian: int32 L; per level array: int32 pyramid level, int32 w, int32 h, then
// w * h float32 pixels; int32 n; per keypoint: float32 x, float32 y, int32 index of its level array.  Printed: one
// line per keypoint, "status angle_bin w0 w1 w2 w3" (the words in hexadecimal), then the program's own checks of a
// constant level (bin 0, no bit set), of the disc list and of the bin rule on the 32 exact directions.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "describe_math.h"

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
  printf("describe_math_check FAILED: %s\n", what);
  return 1;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) return Fail("usage: describe_math_check <cases>");
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
  int32_t n = 0;
  if (!Get(f, &n) || n < 0 || n > sg::kDescMaxKeypoints) return Fail("bad keypoint count");
  for (int i = 0; i < n; ++i) {
    float xy[2];
    int32_t li;
    if (!Get(f, xy, 2) || !Get(f, &li) || li < 0 || li >= L) return Fail("bad keypoint");
    uint64_t d[4];
    int32_t bin;
    const Level& l = lv[li];
    const int st = sg::DescribeOne(l.px.data(), l.w, l.h, l.level, xy[0], xy[1], d, &bin);
    printf("%d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", st, (int)bin, d[0], d[1], d[2], d[3]);
  }
  fclose(f);

  // the disc list: 709 pixels in row-major order, each inside the radius, then (0, 0) padding
  for (int i = 0; i < sg::kDescLanes * sg::kDescPerLane; ++i) {
    const int u = sg::kDescDisc.u[i], v = sg::kDescDisc.v[i];
    if (i >= sg::kDescDiscCount) {
      if (u != 0 || v != 0) return Fail("disc padding is not (0, 0)");
      continue;
    }
    if (u * u + v * v > sg::kDescRadius * sg::kDescRadius) return Fail("disc offset outside the radius");
    if (i > 0) {
      const int pu = sg::kDescDisc.u[i - 1], pv = sg::kDescDisc.v[i - 1];
      if (!(v > pv || (v == pv && u > pu))) return Fail("disc offsets out of order");
    }
  }
  // a constant level: zero moments, so bin 0, and every comparison a tie, so no bit
  {
    std::vector<float> flat(40 * 33, 0.7f);
    uint64_t d[4];
    int32_t bin = -2;
    if (sg::DescribeOne(flat.data(), 40, 33, 0, 20.f, 16.f, d, &bin) != sg::kDescOk) return Fail("constant level refused");
    if (bin != 0 || d[0] || d[1] || d[2] || d[3]) return Fail("constant level: bin 0 and no bit expected");
    if (sg::DescribeOne(flat.data(), 40, 33, 0, 20.f, 18.f, d, &bin) != sg::kDescBorder || bin != -1 || d[0] || d[3])
      return Fail("border keypoint: refusal, bin -1 and zero words expected");
  }
  // the bin rule on its own directions, on the zero centroid and on the axes
  for (int k = 0; k < sg::kBriefBins; ++k)
    if (sg::DescBin(3.0 * sg::kBriefCos[k], 3.0 * sg::kBriefSin[k]) != k) return Fail("bin of its own direction");
  if (sg::DescBin(0.0, 0.0) != 0 || sg::DescBin(-0.0, 0.0) != 0) return Fail("bin of the zero centroid");
  if (sg::DescBin(1.0, 0.0) != 0 || sg::DescBin(0.0, 1.0) != 8 || sg::DescBin(-1.0, 0.0) != 16 ||
      sg::DescBin(0.0, -1.0) != 24)
    return Fail("bins of the axes");
  // the table turns with the pattern: direction k + 8 is the exact quarter turn of direction k
  for (int k = 0; k < sg::kBriefBins; ++k) {
    const int q = (k + 8) % sg::kBriefBins;
    if (sg::kBriefCos[q] != -sg::kBriefSin[k] || sg::kBriefSin[q] != sg::kBriefCos[k]) return Fail("direction table");
  }
  printf("describe_math_check OK\n");
  return 0;
}
