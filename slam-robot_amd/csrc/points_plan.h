// points_plan.h — the host-only planner of sg_slam_solve_points (structure-only bundle adjustment, ba_points.hip):
// from an sg_map and a list of points, everything k_point_lm reads.  A pure function of its arguments (no HIP, no
// environment, no state, no I/O), so a CPU test can recompute it by brute force (tests/native/points_plan_check.cpp).
//
// Per listed point: its enabled observations (obs_disabled == 0, from whatever frame; point flags are NOT
// consulted, unlike sg_problem_from_map_frames' slam-usable filter) in map order, as 24-byte records that name
// their frame by index; its homogeneous location at entry.  The poses are uploaded once per frame in a 64-byte
// table, not gathered per record, so the upload is 24 bytes per observation used plus the frame table and the
// cameras.  A point with fewer than kPointMinObs enabled observations is not solved (one ray does not fix a
// depth): decided here, before anything is launched.
#ifndef SG_POINTS_PLAN_H_
#define SG_POINTS_PLAN_H_

#include <cstdint>
#include <vector>

#include "slamgpu.h"

namespace sg {

constexpr int kPointMinObs = 2;
// sg_slam_triangulate_points (triangulate_math.h): the least gap between the two smallest eigenvalues of the 4x4
// DLT matrix, relative to the largest, at which the null direction counts as determined.  Rounding leaves about
// 1e-16 of the largest eigenvalue in every other one, so below 1e-12 the eigenvector is noise to 1e-4 or worse.
constexpr double kTriMinRelGap = 1e-12;

// One enabled observation of a listed point: the observed pixel and the map index of the observing frame.
struct PointObs {
  double u, v;
  int32_t frame;
  int32_t pad;
};
static_assert(sizeof(PointObs) == 24, "k_point_lm reads records as 2 doubles and 2 ints");

// One frame of the map (all of them constant in this problem).
struct PointFrame {
  double q[4], t[3];   // the pose at entry (Eigen [x,y,z,w] memory)
  int32_t camera;      // index into PointsPlan::k
  int32_t pad;
};
static_assert(sizeof(PointFrame) == 64, "k_point_lm reads frames as 7 doubles and 2 ints");

// One listed point.
struct PointStart {
  double X[4];   // the homogeneous location at entry
  int32_t run;   // 0: fewer than kPointMinObs enabled observations (SG_DID_NOT_RUN, its lanes stay idle)
  int32_t pad;
};
static_assert(sizeof(PointStart) == 40, "k_point_lm reads points as 4 doubles and 2 ints");

struct PointsPlan {
  std::vector<int32_t> off;          // [n + 1] records of listed point i: off[i] .. off[i + 1]
  std::vector<PointObs> obs;         // [off[n]]
  std::vector<PointFrame> frames;    // [num_frames]
  std::vector<double> k;             // [num_cameras][7]
  std::vector<PointStart> points;    // [n]
  int num_run = 0;                   // points with run = 1
};

// Throws sg::Error(SG_EINVAL) on a point index out of range or listed twice and on a map whose indices are out
// of range.  n >= 0; points may be null when n == 0.
void PlanPoints(const sg_map& m, const int32_t* points, int32_t n, PointsPlan* out);

}  // namespace sg

#endif  // SG_POINTS_PLAN_H_
