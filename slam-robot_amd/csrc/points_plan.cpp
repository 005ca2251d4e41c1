// points_plan.cpp — see points_plan.h.
#include "points_plan.h"

#include <cstring>

#include "common.h"

namespace sg {

void PlanPoints(const sg_map& m, const int32_t* points, int32_t n, PointsPlan* out) {
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative point count");
  SG_REQUIRE(n == 0 || points, SG_EINVAL, "null point list");
  SG_REQUIRE(m.num_frames >= 0 && m.num_points >= 0 && m.num_obs >= 0 && m.num_cameras >= 0, SG_EINVAL,
             "negative map sizes");
  const int F = m.num_frames, P = m.num_points, M = m.num_obs;
  out->off.assign((size_t)n + 1, 0);
  out->obs.clear();
  out->frames.clear();
  out->k.clear();
  out->points.assign((size_t)n, PointStart{});
  out->num_run = 0;
  if (n == 0) return;
  // slot[p]: position of point p in the request, -1: not requested
  std::vector<int32_t> slot((size_t)P, -1);
  for (int i = 0; i < n; ++i) {
    const int p = points[i];
    SG_REQUIRE(p >= 0 && p < P, SG_EINVAL, "point index out of range");
    SG_REQUIRE(slot[p] < 0, SG_EINVAL, "point listed twice");
    slot[p] = i;
  }
  // pass 1: enabled observations per requested point (the map's observations are not grouped by point)
  std::vector<int32_t>& off = out->off;
  for (int o = 0; o < M; ++o) {
    const int p = m.obs_point[o], f = m.obs_frame[o];
    SG_REQUIRE(p >= 0 && p < P, SG_EINVAL, "obs_point out of range");
    SG_REQUIRE(f >= 0 && f < F, SG_EINVAL, "obs_frame out of range");
    if (slot[p] >= 0 && m.obs_disabled[o] == 0) off[slot[p] + 1] += 1;
  }
  for (int i = 0; i < n; ++i) off[i + 1] += off[i];
  // pass 2: the records, in map order within each point
  out->obs.resize((size_t)off[n]);
  std::vector<int32_t> fill(off.begin(), off.end() - 1);
  for (int o = 0; o < M; ++o) {
    const int i = slot[m.obs_point[o]];
    if (i < 0 || m.obs_disabled[o] != 0) continue;
    PointObs& r = out->obs[(size_t)fill[i]++];
    r.u = m.obs_pt[2 * (size_t)o];
    r.v = m.obs_pt[2 * (size_t)o + 1];
    r.frame = m.obs_frame[o];
    r.pad = 0;
  }
  out->frames.resize((size_t)F);
  for (int f = 0; f < F; ++f) {
    SG_REQUIRE(m.frame_camera[f] >= 0 && m.frame_camera[f] < m.num_cameras, SG_EINVAL, "frame_camera out of range");
    PointFrame& pf = out->frames[f];
    std::memcpy(pf.q, m.q + 4 * (size_t)f, sizeof(pf.q));
    std::memcpy(pf.t, m.t + 3 * (size_t)f, sizeof(pf.t));
    pf.camera = m.frame_camera[f];
    pf.pad = 0;
  }
  out->k.assign(m.k, m.k + 7 * (size_t)m.num_cameras);
  for (int i = 0; i < n; ++i) {
    PointStart& ps = out->points[i];
    std::memcpy(ps.X, m.X + 4 * (size_t)points[i], sizeof(ps.X));
    ps.run = off[i + 1] - off[i] >= kPointMinObs;
    out->num_run += ps.run;
  }
}

}  // namespace sg
