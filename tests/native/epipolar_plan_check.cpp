// CPU check of csrc/epipolar_plan.cpp, the host-only planner of sg_slam_match_epipolar: on generated maps, the pair
// records against a restatement in plain loops, the preparation, work and merge lists and the partial-result layout
// against brute force (every (a keypoint, b keypoint) of a live pair in exactly one work item, every partial slot
// written by exactly one lane), the 128 MiB cap, ResolveEpipolar against a brute-force restatement of the acceptance
// and uniqueness rule, the CPU executor against an independent double loop, the padding record against the gate, the
// empty shapes, and every SG_EINVAL case of the contract.  Prints the constants that tests/epipolar_cases.py restates.
// Built with epipolar_plan.cpp and match_plan.cpp (ResolveMatches) into one program under AddressSanitizer and UBSan
// by tests/test_epipolar_plan.py.  No GPU, no HIP.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "epipolar_plan.h"

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
  double unit() { return (double)(next() % 2000001) / 1e6 - 1.0; }
};

const double kNaN = std::numeric_limits<double>::quiet_NaN();
const double kInf = std::numeric_limits<double>::infinity();

// Frames looking down +z from centres spread in x and z, small rotations, two cameras (one distorted).
struct Map {
  std::vector<double> k, q, t;
  std::vector<int32_t> cam;
  sg_map m{};
  Map(int F, uint64_t seed) {
    Lcg r{seed};
    k = {0.0, 0.0, 0.0, 416.0, -416.0, 320.0, 240.0, -0.05, 0.01, -0.002, 380.0, -380.0, 330.0, 230.0};
    q.resize(4 * (size_t)F);
    t.resize(3 * (size_t)F);
    cam.resize(F);
    for (int f = 0; f < F; ++f) {
      for (int c = 0; c < 3; ++c) q[4 * f + c] = 0.02 * r.unit();
      q[4 * f + 3] = 1.0 + 0.01 * r.unit();   // not normalised
      t[3 * f] = 150.0 * f + 20.0 * r.unit();
      t[3 * f + 1] = 10.0 * r.unit();
      t[3 * f + 2] = 50.0 * r.unit();
      cam[f] = f % 2;
    }
    m.num_cameras = 2;
    m.k = k.data();
    m.num_frames = F;
    m.q = q.data();
    m.t = t.data();
    m.frame_camera = cam.data();
  }
};

sg_epipolar_options defaults() {
  sg_epipolar_options o{};
  o.tol_px = 2.0;
  o.min_parallax = 0.0;
  o.max_dist = 64;
  o.ratio_percent = 80;
  return o;
}

struct Call {
  std::vector<int32_t> pairs, ao, bo, al, bl;
  std::vector<double> axy, bxy;
  std::vector<uint64_t> ad, bd;
  int n() const { return (int)pairs.size() / 2; }
};

// Keypoints over the image with some NaN pixels; descriptors of 10 random bits so that distances tie.
void fill_side(Lcg& r, int K, std::vector<double>* xy, std::vector<uint64_t>* d, std::vector<int32_t>* lv) {
  xy->assign(2 * (size_t)K + 2, 1.0);
  d->assign(4 * (size_t)K + 4, 0u);
  lv->assign((size_t)K + 1, 0);
  for (int k = 0; k < K; ++k) {
    (*xy)[2 * k] = 320.0 + 320.0 * r.unit();
    (*xy)[2 * k + 1] = 240.0 + 240.0 * r.unit();
    if (r.next() % 97 == 0) (*xy)[2 * k + (r.next() & 1)] = kNaN;
    (*d)[4 * k] = r.next() % 1024;
    (*lv)[k] = (int32_t)(r.next() % 8);
  }
}

Call make_call(const Map& map, const std::vector<int>& na, const std::vector<int>& nb, uint64_t seed) {
  Lcg r{seed};
  Call c;
  c.ao.push_back(0);
  c.bo.push_back(0);
  for (size_t i = 0; i < na.size(); ++i) {
    const int fa = (int)(r.next() % map.m.num_frames);
    int fb = (int)(r.next() % (map.m.num_frames - 1));
    if (fb >= fa) ++fb;
    c.pairs.push_back(fa);
    c.pairs.push_back(fb);
    c.ao.push_back(c.ao.back() + na[i]);
    c.bo.push_back(c.bo.back() + nb[i]);
  }
  fill_side(r, c.ao.back(), &c.axy, &c.ad, &c.al);
  fill_side(r, c.bo.back(), &c.bxy, &c.bd, &c.bl);
  return c;
}

int plan_code(const sg_map* m, const int32_t* pairs, int n, const int32_t* ao, const double* axy, const uint64_t* ad,
              const int32_t* al, const int32_t* bo, const double* bxy, const uint64_t* bd, const int32_t* bl,
              const sg_epipolar_options* o, sg::EpipolarPlan* keep = nullptr) {
  sg::EpipolarPlan plan;
  try {
    sg::PlanEpipolar(m, pairs, n, ao, axy, ad, al, bo, bxy, bd, bl, o, &plan);
  } catch (const sg::Error& e) {
    return e.code;
  }
  if (keep) *keep = plan;
  return SG_OK;
}

int plan_code(const sg_map* m, const Call& c, bool levels, const sg_epipolar_options* o,
              sg::EpipolarPlan* keep = nullptr) {
  return plan_code(m, c.pairs.data(), c.n(), c.ao.data(), c.axy.data(), c.ad.data(), levels ? c.al.data() : nullptr,
                   c.bo.data(), c.bxy.data(), c.bd.data(), levels ? c.bl.data() : nullptr, o, keep);
}

// Step 1 of the contract in plain loops.
struct Record {
  double E[9], R[9], tr[3];
  bool degenerate;
};

void rotation(const double* q, double (*R)[3]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0][0] = 1 - 2 * (y * y + z * z); R[0][1] = 2 * (x * y - w * z);     R[0][2] = 2 * (x * z + w * y);
  R[1][0] = 2 * (x * y + w * z);     R[1][1] = 1 - 2 * (x * x + z * z); R[1][2] = 2 * (y * z - w * x);
  R[2][0] = 2 * (x * z - w * y);     R[2][1] = 2 * (y * z + w * x);     R[2][2] = 1 - 2 * (x * x + y * y);
}

Record record(const sg_map& m, int fa, int fb) {
  double Ra[3][3], Rb[3][3];
  rotation(m.q + 4 * fa, Ra);
  rotation(m.q + 4 * fb, Rb);
  Record r{};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) r.R[3 * i + j] += Rb[i][k] * Ra[j][k];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) r.tr[i] += Rb[i][k] * (m.t[3 * fa + k] - m.t[3 * fb + k]);
  const double tx[3][3] = {{0, -r.tr[2], r.tr[1]}, {r.tr[2], 0, -r.tr[0]}, {-r.tr[1], r.tr[0], 0}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) r.E[3 * i + j] += tx[i][k] * r.R[3 * k + j];
  bool finite = true, zero = true;
  for (int i = 0; i < 9; ++i) {
    finite = finite && std::isfinite(r.E[i]) && std::isfinite(r.R[i]);
    zero = zero && r.E[i] == 0.0;
  }
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(r.tr[i]);
  r.degenerate = !finite || zero;
  return r;
}

bool close(double a, double b, double scale) {
  if (!std::isfinite(a) || !std::isfinite(b)) return !std::isfinite(a) && !std::isfinite(b);   // (a pose that is not finite)
  return std::fabs(a - b) <= 1e-12 * scale;
}

void check_plan(const Map& map, const Call& c, bool levels) {
  const sg_epipolar_options o = defaults();
  sg::EpipolarPlan plan;
  const int code = plan_code(&map.m, c, levels, &o, &plan);
  CHECK(code == SG_OK, "plan failed with %d", code);
  if (code != SG_OK) return;
  const int n = c.n(), KA = c.ao.back(), KB = c.bo.back();
  CHECK(plan.n == n && plan.KA == KA && plan.KB == KB && plan.levels == levels, "sizes");
  CHECK((int)plan.pairs.size() == n && (int)plan.live.size() == n, "array sizes");
  int64_t partials = 0;
  bool any = false;
  for (int i = 0; i < n; ++i) {
    const int fa = c.pairs[2 * i], fb = c.pairs[2 * i + 1];
    const Record r = record(map.m, fa, fb);
    const sg::EpiPair& p = plan.pairs[i];
    double tn = 0.0;
    for (int k = 0; k < 3; ++k) tn = std::fmax(tn, std::fabs(r.tr[k]));
    for (int k = 0; k < 9; ++k)
      CHECK(close(p.E[k], r.E[k], tn) && close(p.R[k], r.R[k], 1.0), "pair %d: E or R entry %d", i, k);
    for (int k = 0; k < 3; ++k) CHECK(close(p.tr[k], r.tr[k], tn), "pair %d: tr", i);
    const double *ka = &map.k[7 * map.cam[fa]], *kb = &map.k[7 * map.cam[fb]];
    CHECK(p.ifa[0] == 1.0 / ka[3] && p.ifa[1] == 1.0 / ka[4] && p.ifb[0] == 1.0 / kb[3] && p.ifb[1] == 1.0 / kb[4],
          "pair %d: inverse focal lengths", i);
    CHECK(std::memcmp(p.ka, ka, 56) == 0 && std::memcmp(p.kb, kb, 56) == 0, "pair %d: cameras", i);
    CHECK((p.degenerate != 0) == r.degenerate, "pair %d: degenerate", i);
    const int na = c.ao[i + 1] - c.ao[i], nb = c.bo[i + 1] - c.bo[i];
    const bool live = !r.degenerate && na > 0 && nb > 0;
    CHECK((plan.live[i] != 0) == live, "pair %d: live", i);
    if (live) partials += (int64_t)na * ((nb + sg::kEpiSlice - 1) / sg::kEpiSlice);
    any = any || live;
  }
  CHECK(plan.partials == partials && plan.launch == any, "partials %lld, want %lld", (long long)plan.partials,
        (long long)partials);
  // the preparation list: every keypoint of a live pair once, none of another pair
  std::vector<int> sa((size_t)KA, 0), sb((size_t)KB, 0);
  for (const sg::EpiPrepItem& it : plan.prep) {
    CHECK(it.pair >= 0 && it.pair < n && (it.side == 0 || it.side == 1) && it.count >= 1 && it.count <= sg::kEpiPrepRun,
          "prep item");
    const std::vector<int32_t>& off = it.side ? c.bo : c.ao;
    CHECK(plan.live[it.pair] && it.k0 >= off[it.pair] && it.k0 + it.count <= off[it.pair + 1], "prep item outside its pair");
    for (int k = it.k0; k < it.k0 + it.count; ++k) ++(it.side ? sb : sa)[k];
  }
  for (int i = 0; i < n; ++i) {
    for (int k = c.ao[i]; k < c.ao[i + 1]; ++k) CHECK(sa[k] == (plan.live[i] ? 1 : 0), "a keypoint %d prepared %d times", k, sa[k]);
    for (int k = c.bo[i]; k < c.bo[i + 1]; ++k) CHECK(sb[k] == (plan.live[i] ? 1 : 0), "b keypoint %d prepared %d times", k, sb[k]);
  }
  // the work list: every (a, b) of a live pair in one item; every partial slot written by one lane of one item
  std::vector<int> slot((size_t)partials, 0);
  std::vector<int64_t> covered((size_t)n, 0);
  int32_t last_pair = -1;
  for (const sg::EpiItem& it : plan.items) {
    CHECK(it.pair >= last_pair && it.pair < n, "item order");
    last_pair = it.pair;
    const int i = it.pair;
    const int na = c.ao[i + 1] - c.ao[i], nb = c.bo[i + 1] - c.bo[i];
    CHECK(plan.live[i] && it.acount >= 1 && it.acount <= sg::kEpiChunk && it.bcount >= 1 && it.bcount <= sg::kEpiSlice,
          "item counts");
    CHECK(it.a0 >= c.ao[i] && it.a0 + it.acount <= c.ao[i + 1] && (it.a0 - c.ao[i]) % sg::kEpiChunk == 0, "item chunk");
    CHECK(it.a0 + it.acount == c.ao[i + 1] || it.acount == sg::kEpiChunk, "a short chunk that is not the last");
    CHECK(it.b0 == c.bo[i] + it.j0 && it.j0 % sg::kEpiSlice == 0 && it.j0 + it.bcount <= nb, "item slice");
    CHECK(it.j0 + it.bcount == nb || it.bcount == sg::kEpiSlice, "a short slice that is not the last");
    covered[i] += (int64_t)it.acount * it.bcount;
    for (int l = 0; l < it.acount; ++l) {
      const int64_t at = (int64_t)it.part0 + l;
      CHECK(at >= 0 && at < partials, "partial slot %lld out of range", (long long)at);
      if (at >= 0 && at < partials) ++slot[at];
    }
    (void)na;
  }
  for (int i = 0; i < n; ++i) {
    const int64_t na = c.ao[i + 1] - c.ao[i], nb = c.bo[i + 1] - c.bo[i];
    CHECK(covered[i] == (plan.live[i] ? na * nb : 0), "pair %d: %lld of %lld candidates covered", i,
          (long long)covered[i], (long long)(na * nb));
  }
  for (int64_t s = 0; s < partials; ++s) CHECK(slot[s] == 1, "partial slot %lld written %d times", (long long)s, slot[s]);
  // the merge list: every a keypoint of a live pair once; its slots are those its items wrote
  std::vector<int> merged((size_t)KA, 0);
  for (const sg::EpiChunkItem& ch : plan.chunks) {
    CHECK(ch.count >= 1 && ch.count <= sg::kEpiChunk && ch.slices >= 1 && ch.stride >= ch.count, "chunk item");
    for (int l = 0; l < ch.count; ++l) {
      if (ch.a0 + l < KA) ++merged[ch.a0 + l];
      for (int s = 0; s < ch.slices; ++s) {
        const int64_t at = (int64_t)ch.part0 + l + (int64_t)s * ch.stride;
        CHECK(at >= 0 && at < partials, "merge slot out of range");
        // the item that wrote it: same chunk, slice s
        bool found = false;
        for (const sg::EpiItem& it : plan.items)
          found = found || (it.a0 == ch.a0 && it.j0 == s * sg::kEpiSlice && it.part0 + l == at);
        CHECK(found, "merge slot %lld of keypoint %d slice %d has no writer", (long long)at, ch.a0 + l, s);
      }
    }
  }
  for (int i = 0; i < n; ++i)
    for (int k = c.ao[i]; k < c.ao[i + 1]; ++k) CHECK(merged[k] == (plan.live[i] ? 1 : 0), "a keypoint %d merged %d times", k, merged[k]);
}

// The CPU executor against an independent double loop that restates steps 2 to 4 from the contract's formulas.
void undistort(const double* k, const double* px, double* x) {
  const double xd = (px[0] - k[5]) / k[3], yd = (px[1] - k[6]) / k[4];
  const double rd = std::sqrt(xd * xd + yd * yd);
  if (rd == 0.0) {
    x[0] = x[1] = 0.0;
    return;
  }
  double r = rd;
  for (int it = 0; it < 8; ++it) {
    const double r2 = r * r;
    r -= (r * (1 + r2 * (k[0] + r2 * (k[1] + r2 * k[2]))) - rd) / (1 + r2 * (3 * k[0] + r2 * (5 * k[1] + r2 * 7 * k[2])));
  }
  x[0] = xd * r / rd;
  x[1] = yd * r / rd;
}

struct Executed {
  int near = 0;   // decisions within 1e-9 relative of their threshold: the two evaluations may differ there
  long candidates = 0;
};

Executed check_executor(const Map& map, const Call& c, bool levels, double tol, double min_parallax) {
  sg_epipolar_options o = defaults();
  o.tol_px = tol;
  o.min_parallax = min_parallax;
  sg::EpipolarPlan plan;
  Executed ex;
  if (plan_code(&map.m, c, levels, &o, &plan) != SG_OK) {
    CHECK(false, "plan failed");
    return ex;
  }
  const int KA = c.ao.back();
  std::vector<int32_t> bk((size_t)KA + 1, 7), bd(bk), sd(bk), nc(bk);
  sg::RunEpipolarCpu(plan, c.ao.data(), c.axy.data(), c.ad.data(), levels ? c.al.data() : nullptr, c.bo.data(),
                     c.bxy.data(), c.bd.data(), levels ? c.bl.data() : nullptr, o, bk.data(), bd.data(), sd.data(),
                     nc.data());
  CHECK(bk[KA] == 7 && bd[KA] == 7 && sd[KA] == 7 && nc[KA] == 7, "wrote past the keypoints");
  for (int i = 0; i < c.n(); ++i) {
    const int fa = c.pairs[2 * i], fb = c.pairs[2 * i + 1];
    const Record r = record(map.m, fa, fb);
    const double *ka = &map.k[7 * map.cam[fa]], *kb = &map.k[7 * map.cam[fb]];
    const int nb = c.bo[i + 1] - c.bo[i];
    for (int k = c.ao[i]; k < c.ao[i + 1]; ++k) {
      double xa[2];
      undistort(ka, &c.axy[2 * k], xa);
      const double fav[3] = {xa[0], xa[1], 1.0};
      double l[3] = {0, 0, 0}, g[3] = {0, 0, 0};
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          l[a] += r.E[3 * a + b] * fav[b];
          g[a] += r.R[3 * a + b] * fav[b];
        }
      const double na = std::pow(l[0] / kb[3], 2) + std::pow(l[1] / kb[4], 2);
      int best = -1, d1 = 1000, d2 = 1000, count = 0;
      bool unsure = false;
      for (int j = 0; j < nb && !r.degenerate; ++j) {
        const int jb = c.bo[i] + j;
        double xb[2];
        undistort(kb, &c.bxy[2 * jb], xb);
        const double fbv[3] = {xb[0], xb[1], 1.0};
        const double m0 = r.E[0] * fbv[0] + r.E[3] * fbv[1] + r.E[6], m1 = r.E[1] * fbv[0] + r.E[4] * fbv[1] + r.E[7];
        const double nbv = std::pow(m0 / ka[3], 2) + std::pow(m1 / ka[4], 2);
        const double res = xb[0] * l[0] + xb[1] * l[1] + l[2];
        const int L = levels ? std::max(c.al[k], c.bl[jb]) : 0;
        const double thr = tol * tol * std::pow(4.0, L) * (na + nbv);
        if (!(na + nbv > 0.0) || !(res * res <= thr)) {
          unsure = unsure || std::fabs(res * res - thr) <= 1e-9 * thr;
          continue;
        }
        unsure = unsure || std::fabs(res * res - thr) <= 1e-9 * thr;
        double gg = 0, gf = 0, ff = 0, gt = 0, ft = 0;
        for (int a = 0; a < 3; ++a) {
          gg += g[a] * g[a];
          gf += g[a] * fbv[a];
          ff += fbv[a] * fbv[a];
          gt += g[a] * r.tr[a];
          ft += fbv[a] * r.tr[a];
        }
        const double det = gg * ff - gf * gf, da = gf * ft - gt * ff, db = gg * ft - gf * gt;
        unsure = unsure || std::fabs(det) <= 1e-9 * gg * ff ||
                 std::fabs(da) <= 1e-9 * (std::fabs(gf * ft) + std::fabs(gt * ff)) ||
                 std::fabs(db) <= 1e-9 * (std::fabs(gg * ft) + std::fabs(gf * gt));
        if (!(det > 0.0 && da > 0.0 && db > 0.0)) continue;
        if (min_parallax > 0.0) {
          const double cx = g[1] * fbv[2] - g[2] * fbv[1], cy = g[2] * fbv[0] - g[0] * fbv[2],
                       cz = g[0] * fbv[1] - g[1] * fbv[0];
          const double par = std::atan2(std::sqrt(cx * cx + cy * cy + cz * cz), gf);
          unsure = unsure || std::fabs(par - min_parallax) <= 1e-9 * min_parallax;
          if (!(par >= min_parallax)) continue;
        }
        int h = 0;
        for (int w = 0; w < 4; ++w) h += __builtin_popcountll(c.ad[4 * (size_t)k + w] ^ c.bd[4 * (size_t)jb + w]);
        ++count;
        if (h < d1) {
          d2 = d1;
          d1 = h;
          best = j;
        } else if (h < d2) {
          d2 = h;
        }
      }
      if (unsure) {
        ++ex.near;
        continue;
      }
      ex.candidates += count;
      CHECK(nc[k] == count && bk[k] == best && bd[k] == (count ? d1 : -1) && sd[k] == (count > 1 ? d2 : -1),
            "pair %d keypoint %d: executor (%d, %d, %d, %d), want (%d, %d, %d, %d)", i, k, bk[k], bd[k], sd[k], nc[k],
            best, count ? d1 : -1, count > 1 ? d2 : -1, count);
    }
  }
  return ex;
}

void check_padding() {
  Map map(4, 3);
  sg::EpiPair p;
  sg::EpiPairFrom(&map.q[0], &map.t[0], &map.k[7], &map.q[4], &map.t[3], &map.k[0], &p);
  const sg::EpiB pad = sg::EpiPadB();
  Lcg r{5};
  for (int i = 0; i < 2000; ++i) {
    double px[2] = {320.0 + 400.0 * r.unit(), 240.0 + 300.0 * r.unit()};
    if (i % 50 == 0) px[i % 2] = i % 100 ? kNaN : kInf;
    sg::EpiA a;
    sg::EpiPrepA(p, px, i % 8, &a);
    CHECK(!sg::EpiGate(a, pad, 1e300) && !sg::EpiCandidate(a, pad, 1e300, 0.0), "the padding record passed the gate");
  }
}

void check_resolve(uint64_t seed, int max_dist, int ratio) {
  Lcg r{seed};
  const int n = 6;
  sg::EpipolarPlan plan;
  plan.n = n;
  plan.pairs.resize(n);
  for (int i = 0; i < n; ++i) plan.pairs[i].degenerate = i == 4;
  std::vector<int32_t> ao(1, 0), bo(1, 0);
  for (int i = 0; i < n; ++i) {
    ao.push_back(ao.back() + (i == 2 ? 0 : (int)(r.next() % 400)));
    bo.push_back(bo.back() + 40);
  }
  const int K = ao.back();
  std::vector<int32_t> bk(K), bd(K), sd(K), nc(K);
  for (int i = 0; i < n; ++i)
    for (int k = ao[i]; k < ao[i + 1]; ++k) {
      nc[k] = i == 4 ? 0 : (int)(r.next() % 4);
      bk[k] = nc[k] ? (int)(r.next() % 40) : -1;   // few b keypoints: many claimants each
      bd[k] = nc[k] ? (int)(r.next() % 90) : -1;
      sd[k] = nc[k] > 1 ? bd[k] + (int)(r.next() % 30) : -1;
    }
  sg_epipolar_options o = defaults();
  o.max_dist = max_dist;
  o.ratio_percent = ratio;
  std::vector<int32_t> match((size_t)K + 1, 7);
  std::vector<sg_epipolar_result> res(n);
  sg::ResolveEpipolar(plan, ao.data(), bo.data(), bk.data(), bd.data(), sd.data(), nc.data(), o, match.data(), res.data());
  CHECK(match[K] == 7, "wrote past the keypoints");
  for (int i = 0; i < n; ++i) {
    int with = 0, matched = 0;
    for (int k = ao[i]; k < ao[i + 1]; ++k) {
      with += nc[k] > 0;
      auto accepted = [&](int a) {
        return bk[a] >= 0 && bd[a] <= max_dist && (sd[a] < 0 || 100 * bd[a] <= ratio * sd[a]);
      };
      int want = -1;
      if (accepted(k)) {
        want = bk[k];
        for (int a = ao[i]; a < ao[i + 1]; ++a)   // a better claimant of the same b keypoint, in this pair only
          if (a != k && accepted(a) && bk[a] == bk[k] && (bd[a] < bd[k] || (bd[a] == bd[k] && a < k))) want = -1;
      }
      CHECK(match[k] == want, "match of keypoint %d: %d, want %d", k, match[k], want);
      matched += want >= 0;
    }
    CHECK(res[i].num_a == ao[i + 1] - ao[i] && res[i].num_b == 40 && res[i].num_with_candidates == with &&
              res[i].num_matched == matched && res[i].degenerate == (i == 4),
          "counts of pair %d", i);
  }
  sg::ResolveEpipolar(plan, ao.data(), bo.data(), bk.data(), bd.data(), sd.data(), nc.data(), o, match.data(), nullptr);
}

void check_errors() {
  Map map(6, 11);
  const Call c = make_call(map, {70, 0, 5, 130}, {600, 9, 0, 300}, 3);
  const sg_epipolar_options o = defaults();
  const int n = c.n();
  const int32_t *pr = c.pairs.data(), *ao = c.ao.data(), *bo = c.bo.data(), *al = c.al.data(), *bl = c.bl.data();
  const double *axy = c.axy.data(), *bxy = c.bxy.data();
  const uint64_t *ad = c.ad.data(), *bd = c.bd.data();
  sg::EpipolarPlan plan;
  CHECK(plan_code(&map.m, c, true, &o) == SG_OK && plan_code(&map.m, c, false, &o) == SG_OK, "the base call");
  CHECK(plan_code(nullptr, pr, n, ao, axy, ad, al, bo, bxy, bd, bl, &o) == SG_EINVAL, "null map");
  CHECK(plan_code(&map.m, pr, n, ao, axy, ad, al, bo, bxy, bd, bl, nullptr) == SG_EINVAL, "null options");
  CHECK(plan_code(&map.m, pr, -1, ao, axy, ad, al, bo, bxy, bd, bl, &o) == SG_EINVAL, "n < 0");
  CHECK(plan_code(&map.m, nullptr, n, ao, axy, ad, al, bo, bxy, bd, bl, &o) == SG_EINVAL, "null pairs");
  CHECK(plan_code(&map.m, pr, n, nullptr, axy, ad, al, bo, bxy, bd, bl, &o) == SG_EINVAL, "null a_offset");
  CHECK(plan_code(&map.m, pr, n, ao, axy, ad, al, nullptr, bxy, bd, bl, &o) == SG_EINVAL, "null b_offset");
  CHECK(plan_code(&map.m, pr, n, ao, nullptr, ad, al, bo, bxy, bd, bl, &o) == SG_EINVAL, "null a_xy");
  CHECK(plan_code(&map.m, pr, n, ao, axy, nullptr, al, bo, bxy, bd, bl, &o) == SG_EINVAL, "null a_desc");
  CHECK(plan_code(&map.m, pr, n, ao, axy, ad, al, bo, nullptr, bd, bl, &o) == SG_EINVAL, "null b_xy");
  CHECK(plan_code(&map.m, pr, n, ao, axy, ad, al, bo, bxy, nullptr, bl, &o) == SG_EINVAL, "null b_desc");
  CHECK(plan_code(&map.m, pr, n, ao, axy, ad, nullptr, bo, bxy, bd, bl, &o) == SG_EINVAL, "levels of b only");
  CHECK(plan_code(&map.m, pr, n, ao, axy, ad, al, bo, bxy, bd, nullptr, &o) == SG_EINVAL, "levels of a only");
  // lists that would not be read may be null: no keypoints on a side, n == 0
  const int32_t zero_off[5] = {0, 0, 0, 0, 0};
  CHECK(plan_code(&map.m, pr, n, zero_off, nullptr, nullptr, nullptr, bo, bxy, bd, nullptr, &o, &plan) == SG_OK &&
            !plan.launch && plan.items.empty() && plan.prep.empty() && plan.chunks.empty() && plan.KA == 0,
        "KA == 0");
  CHECK(plan_code(&map.m, pr, n, ao, axy, ad, nullptr, zero_off, nullptr, nullptr, nullptr, &o, &plan) == SG_OK &&
            !plan.launch && plan.items.empty() && plan.partials == 0,
        "KB == 0");
  CHECK(plan_code(&map.m, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &o, &plan) ==
                SG_OK && !plan.launch && plan.pairs.empty(),
        "n == 0");
  for (int side = 0; side < 2; ++side) {
    std::vector<int32_t> b(side ? c.bo : c.ao);
    b[0] = 1;
    CHECK(plan_code(&map.m, pr, n, side ? ao : b.data(), axy, ad, al, side ? b.data() : bo, bxy, bd, bl, &o) == SG_EINVAL,
          "offset[0] != 0");
    b = side ? c.bo : c.ao;
    b[2] = b[1] - 1;
    CHECK(plan_code(&map.m, pr, n, side ? ao : b.data(), axy, ad, al, side ? b.data() : bo, bxy, bd, bl, &o) == SG_EINVAL,
          "decreasing offset");
    const int32_t big[2] = {0, sg::kEpiMaxKeypoints + 1}, small[2] = {0, 1};
    CHECK(plan_code(&map.m, pr, 1, side ? small : big, axy, ad, nullptr, side ? big : small, bxy, bd, nullptr, &o) ==
              SG_EINVAL,
          "more than 2^20 keypoints");   // (found before the arrays are read)
    for (int32_t bad : {-1, 8}) {
      std::vector<int32_t> lv(side ? c.bl : c.al);
      lv[3] = bad;
      CHECK(plan_code(&map.m, pr, n, ao, axy, ad, side ? al : lv.data(), bo, bxy, bd, side ? lv.data() : bl, &o) == SG_EINVAL,
            "level %d", bad);
    }
  }
  for (int slot = 0; slot < 2; ++slot)
    for (int32_t bad : {-1, 6, 0x7fffffff}) {
      std::vector<int32_t> b(c.pairs);
      b[4 + slot] = bad;
      CHECK(plan_code(&map.m, b.data(), n, ao, axy, ad, al, bo, bxy, bd, bl, &o) == SG_EINVAL, "frame %d", bad);
    }
  {
    std::vector<int32_t> b(c.pairs);
    b[3] = b[2];
    CHECK(plan_code(&map.m, b.data(), n, ao, axy, ad, al, bo, bxy, bd, bl, &o) == SG_EINVAL, "a == b");
  }
  auto with = [&](auto set) {
    sg_epipolar_options b = defaults();
    set(b);
    // option errors are found with n == 0 too
    return plan_code(&map.m, pr, n, ao, axy, ad, al, bo, bxy, bd, bl, &b) == SG_EINVAL &&
           plan_code(&map.m, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &b) == SG_EINVAL;
  };
  for (double bad : {0.0, -1.0, kNaN, kInf, -kInf})
    CHECK(with([&](sg_epipolar_options& b) { b.tol_px = bad; }), "tol_px %g", bad);
  for (double bad : {-1e-9, kNaN, kInf, -kInf})
    CHECK(with([&](sg_epipolar_options& b) { b.min_parallax = bad; }), "min_parallax %g", bad);
  for (int bad : {-1, 257}) CHECK(with([&](sg_epipolar_options& b) { b.max_dist = bad; }), "max_dist %d", bad);
  for (int bad : {0, -5, 101}) CHECK(with([&](sg_epipolar_options& b) { b.ratio_percent = bad; }), "ratio_percent %d", bad);
  for (int ok : {0, 256}) {
    sg_epipolar_options b = defaults();
    b.max_dist = ok;
    b.ratio_percent = ok ? 100 : 1;
    b.min_parallax = ok ? 0.5 : 0.0;
    CHECK(plan_code(&map.m, c, true, &b) == SG_OK, "the ends of the ranges are valid");
  }
  {   // the cap: 2^13 a keypoints against 2^10 slices is 2^23 partial results and passes; one more slice does not
    const int32_t a13[2] = {0, 1 << 13}, b_ok[2] = {0, sg::kEpiSlice << 10}, b_over[2] = {0, (sg::kEpiSlice << 10) + 1};
    std::vector<double> xy(2u << 19, 1.0);
    std::vector<uint64_t> d(4u << 19, 1u);
    CHECK(plan_code(&map.m, pr, 1, a13, xy.data(), d.data(), nullptr, b_ok, xy.data(), d.data(), nullptr, &o, &plan) == SG_OK &&
              plan.partials == sg::kEpiMaxPartials && (int64_t)plan.items.size() == (int64_t)(1 << 7) << 10,
          "2^23 partial results");
    CHECK(plan_code(&map.m, pr, 1, a13, xy.data(), d.data(), nullptr, b_over, xy.data(), d.data(), nullptr, &o) == SG_EINVAL,
          "more than 2^23 partial results");
    // the cap is over the sum of the pairs: two pairs of 2^13 x 2^9 slices pass, with one b keypoint more they do not
    const int32_t pr2[4] = {0, 1, 2, 3}, a2[3] = {0, 1 << 13, 1 << 14};
    const int32_t b2_ok[3] = {0, sg::kEpiSlice << 9, sg::kEpiSlice << 10};
    const int32_t b2_over[3] = {0, sg::kEpiSlice << 9, (sg::kEpiSlice << 10) + 1};
    CHECK(plan_code(&map.m, pr2, 2, a2, xy.data(), d.data(), nullptr, b2_ok, xy.data(), d.data(), nullptr, &o, &plan) == SG_OK &&
              plan.partials == sg::kEpiMaxPartials,
          "two pairs at the cap");
    CHECK(plan_code(&map.m, pr2, 2, a2, xy.data(), d.data(), nullptr, b2_over, xy.data(), d.data(), nullptr, &o) == SG_EINVAL,
          "two pairs above the cap");
  }
  // maps that cannot be read
  auto broken = [&](auto set) {
    Map b(6, 11);
    set(b);
    return plan_code(&b.m, c, true, &o);
  };
  CHECK(broken([](Map& b) { b.m.q = nullptr; }) == SG_EINVAL, "null q");
  CHECK(broken([](Map& b) { b.m.t = nullptr; }) == SG_EINVAL, "null t");
  CHECK(broken([](Map& b) { b.m.k = nullptr; }) == SG_EINVAL, "null k");
  CHECK(broken([](Map& b) { b.m.frame_camera = nullptr; }) == SG_EINVAL, "null frame_camera");
  CHECK(broken([&](Map& b) { b.cam[c.pairs[1]] = 2; }) == SG_EINVAL, "camera out of range");
  CHECK(broken([&](Map& b) { b.cam[c.pairs[0]] = -1; }) == SG_EINVAL, "negative camera");
  CHECK(broken([](Map& b) { b.m.num_frames = -1; }) == SG_EINVAL, "negative num_frames");
  // the planner needs neither points nor observations (null in Map); a pose that is not finite is no error
  CHECK(broken([&](Map& b) { b.t[3 * c.pairs[0]] = kNaN; }) == SG_OK, "a NaN pose makes a degenerate pair");
}

void check_degenerate() {
  Map map(6, 21);
  std::memcpy(&map.t[3 * 3], &map.t[3 * 2], 24);   // frames 2 and 3 share a centre
  map.q[4 * 5] = kInf;
  Call c = make_call(map, {20, 20, 20}, {30, 30, 30}, 9);
  const int32_t pairs[6] = {2, 3, 0, 5, 0, 1};
  c.pairs.assign(pairs, pairs + 6);
  const sg_epipolar_options o = defaults();
  sg::EpipolarPlan plan;
  CHECK(plan_code(&map.m, c, false, &o, &plan) == SG_OK, "plan");
  CHECK(plan.pairs[0].degenerate == 1 && plan.pairs[1].degenerate == 1 && plan.pairs[2].degenerate == 0 &&
            !plan.live[0] && !plan.live[1] && plan.live[2] && plan.partials == 20 && plan.items.size() == 1,
        "zero baseline and non-finite pose");
  check_plan(map, c, false);
  check_executor(map, c, false, 30.0, 0.0);
}

}  // namespace

int main() {
  std::printf("kEpiChunk %d kEpiTile %d kEpiSlice %d kEpiKeyShift %d\n", sg::kEpiChunk, sg::kEpiTile, sg::kEpiSlice,
              sg::kEpiKeyShift);
  Map map(8, 1);
  const Call big = make_call(map, {1, 63, 64, 65, 130, 0, 300, 7}, {1, 3, 255, 256, 257, 40, 2 * sg::kEpiSlice + 76, 0}, 2);
  check_plan(map, big, true);
  check_plan(map, big, false);
  check_plan(map, make_call(map, {1}, {1}, 3), false);
  check_plan(map, make_call(map, {sg::kEpiChunk * 3}, {sg::kEpiSlice}, 4), true);
  check_plan(map, make_call(map, {5, 5}, {sg::kEpiSlice + 1, sg::kEpiSlice * 3}, 5), true);
  Executed ex{};
  for (int v = 0; v < 4; ++v) {
    const Executed e = check_executor(map, big, v & 1, v & 2 ? 25.0 : 2.0, v & 2 ? 0.02 : 0.0);
    ex.near += e.near;
    ex.candidates += e.candidates;
  }
  std::printf("executor: %ld candidates compared, %d keypoints skipped near a threshold\n", ex.candidates, ex.near);
  CHECK(ex.candidates > 1000 && ex.near < 5, "the executor check compared too little");
  check_padding();
  for (uint64_t s = 1; s <= 4; ++s) check_resolve(s, 64, 80);
  check_resolve(9, 0, 100);
  check_resolve(10, 256, 1);
  check_errors();
  check_degenerate();
  if (g_fail) {
    std::printf("epipolar_plan_check FAILED: %d checks\n", g_fail);
    return 1;
  }
  std::printf("epipolar_plan_check OK\n");
  return 0;
}
