// pose_plan.cpp — see pose_plan.h.
#include "pose_plan.h"

#include <cstring>

#include "common.h"

namespace sg {

namespace {
// TrackedPoint::slam_usable (localmap.h:242-248), as problem.cpp's kUnusableMask
constexpr int kPoseUnusableMask =
    (1 << SG_BAD_LOCATION) | (1 << SG_NO_BASELINE) | (1 << SG_NO_OBSERVATIONS) | (1 << SG_BAD_FEATURE);
}  // namespace

void PlanPoses(const sg_map& m, const int32_t* frames, int32_t n, bool with_frame_distance, PosePlan* out,
               int min_obs, bool with_obs_index) {
  SG_REQUIRE(n >= 0, SG_EINVAL, "negative frame count");
  SG_REQUIRE(n == 0 || frames, SG_EINVAL, "null frame list");
  SG_REQUIRE(m.num_frames >= 0 && m.num_points >= 0 && m.num_obs >= 0 && m.num_cameras >= 0, SG_EINVAL,
             "negative map sizes");
  const int F = m.num_frames, P = m.num_points, M = m.num_obs;
  out->off.assign((size_t)n + 1, 0);
  out->records.clear();
  out->obs.clear();
  out->frames.assign((size_t)n, PoseFrame{});
  out->num_run = 0;
  if (n == 0) return;
  // slot[f]: position of frame f in the request, -1: not requested
  std::vector<int32_t> slot((size_t)F, -1);
  for (int i = 0; i < n; ++i) {
    const int f = frames[i];
    SG_REQUIRE(f >= 0 && f < F, SG_EINVAL, "frame index out of range");
    SG_REQUIRE(slot[f] < 0, SG_EINVAL, "frame listed twice");
    SG_REQUIRE(m.frame_camera[f] >= 0 && m.frame_camera[f] < m.num_cameras, SG_EINVAL, "frame_camera out of range");
    SG_REQUIRE(m.frame_prev[f] >= -1 && m.frame_prev[f] < F, SG_EINVAL, "frame_prev out of range");
    slot[f] = i;
  }
  // pass 1: usable observations per requested frame (the map's observations need not be grouped by frame)
  auto usable = [&](int o) {
    const int pt = m.obs_point[o];
    SG_REQUIRE(pt >= 0 && pt < P, SG_EINVAL, "obs_point out of range");
    return m.obs_disabled[o] == 0 && (m.point_flags[pt] & kPoseUnusableMask) == 0;
  };
  std::vector<int32_t>& off = out->off;
  for (int o = 0; o < M; ++o) {
    const int f = m.obs_frame[o];
    SG_REQUIRE(f >= 0 && f < F, SG_EINVAL, "obs_frame out of range");
    if (slot[f] >= 0 && usable(o)) off[slot[f] + 1] += 1;
  }
  for (int i = 0; i < n; ++i) off[i + 1] += off[i];
  // pass 2: the records, in map order within each frame
  out->records.resize((size_t)off[n]);
  if (with_obs_index) out->obs.resize((size_t)off[n]);
  std::vector<int32_t> fill(off.begin(), off.end() - 1);
  for (int o = 0; o < M; ++o) {
    const int i = slot[m.obs_frame[o]];
    if (i < 0 || !usable(o)) continue;
    if (with_obs_index) out->obs[(size_t)fill[i]] = o;
    PoseRecord& r = out->records[(size_t)fill[i]++];
    r.u = m.obs_pt[2 * (size_t)o];
    r.v = m.obs_pt[2 * (size_t)o + 1];
    std::memcpy(r.X, m.X + 4 * (size_t)m.obs_point[o], sizeof(r.X));
  }
  for (int i = 0; i < n; ++i) {
    const int f = frames[i];
    PoseFrame& pf = out->frames[i];
    std::memcpy(pf.q, m.q + 4 * (size_t)f, sizeof(pf.q));
    std::memcpy(pf.t, m.t + 3 * (size_t)f, sizeof(pf.t));
    std::memcpy(pf.k, m.k + 7 * (size_t)m.frame_camera[f], sizeof(pf.k));
    const int prev = m.frame_prev[f];
    pf.has_dist = with_frame_distance && prev >= 0;
    if (prev >= 0) std::memcpy(pf.tprev, m.t + 3 * (size_t)prev, sizeof(pf.tprev));
    pf.run = off[i + 1] - off[i] >= min_obs;
    out->num_run += pf.run;
  }
}

}  // namespace sg
