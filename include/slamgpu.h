/*
 * slamgpu.h — C-ABI of the MI355X-native local-mapping back end (libslamgpu.so).
 *
 * The drop-in boundary for the reference's hot path (ywrt/slam-robot):
 *   - class Slam            (slam.h:21-65)  -> sg_slam_* (SolveFrames / SolveAllFrames / ReprojectMap,
 *                                              iterations(), error())
 *   - Ceres problem + solve (slam.cpp:257-521) -> sg_problem_* / sg_ba_*  (compact problem, LM solve)
 *   - ProjectPoint          (project.h:11-54) -> device code inside the solver and sg_project_points
 *   - HessianTracker        (hessian.h:9-270) -> sg_tracker_*           (front end, see sg_track_*)
 *
 * Conventions: plain pointers and sizes only, no C++/torch types.  Every entry point returns 0 (SG_OK) on
 * success or a negative errno-style code.  The caller owns every host array it passes; the library owns
 * its device buffers (allocated on first use, grown on demand, freed by *_destroy).  One handle per host
 * thread; each handle owns one HIP stream on the device named in its options.
 */
#ifndef SLAMGPU_H_
#define SLAMGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_OK 0
#define SG_EINVAL (-22)   /* bad argument / inconsistent sizes */
#define SG_ENOMEM (-12)   /* host or device allocation failed */
#define SG_EDEVICE (-5)   /* HIP runtime error (message via sg_last_error) */
#define SG_ENODEV (-19)   /* no usable gfx950 device */
#define SG_ECOMM (-71)    /* RCCL error */

/* Bit positions of TrackedPoint::Flags (localmap.h:184-190). point_flags holds (1 << flag). */
enum sg_point_flag {
  SG_BAD_LOCATION = 0,
  SG_NO_BASELINE = 1,
  SG_NO_OBSERVATIONS = 2,
  SG_MISMATCHED = 3,
  SG_BAD_FEATURE = 4
};

/* Termination types (ceres::SolverTerminationType, Ceres 1.8 naming). */
enum sg_termination {
  SG_NO_CONVERGENCE = 0,
  SG_FUNCTION_TOLERANCE = 1,
  SG_GRADIENT_TOLERANCE = 2,
  SG_PARAMETER_TOLERANCE = 3,
  SG_NUMERICAL_FAILURE = 4,
  SG_DID_NOT_RUN = 5,
  SG_DEVICE_TIMEOUT = 6   /* not a Ceres type: a device hand-off of the Cholesky hit its spin limit (the GPU was
                             shared or stalled); the step is not trusted and the solve fails (ok = 0) */
};

/*
 * LocalMap (localmap.h:284-320) in structure-of-arrays form.  Frames are in LocalMap::frames order,
 * observations grouped by frame in Frame::observations() order.  q/t/X/k are the parameter blocks the
 * reference hands to Ceres by raw pointer (localmap.h:129-132,159-160,194-195,30); they are updated in
 * place by a solve exactly as Ceres updates the map's own storage.
 */
typedef struct sg_map {
  int32_t num_cameras;
  double* k;                    /* [7*num_cameras]  Camera::k = k1,k2,k3,fx,fy,cx,cy */
  int32_t num_frames;
  double* q;                    /* [4*F] Frame::rotation().coeffs()  Eigen order [x,y,z,w] */
  double* t;                    /* [3*F] Frame::translation() */
  const int32_t* frame_camera;  /* [F] index into cameras */
  const int32_t* frame_prev;    /* [F] index of Frame::previous(), -1 if none */
  int32_t num_points;
  double* X;                    /* [4*P] TrackedPoint::location() homogeneous [X,Y,Z,W] */
  int32_t* point_flags;         /* [P] TrackedPoint flags bitmask */
  double* point_uncertainty;    /* [P] TrackedPoint::uncertainty() */
  int32_t num_obs;
  const double* obs_pt;         /* [2*M] Observation::pt (pixels) */
  const int32_t* obs_frame;     /* [M] */
  const int32_t* obs_point;     /* [M] */
  int32_t* obs_disabled;        /* [M] Observation::is_disabled */
  double* obs_error;            /* [2*M] Observation::error, written by ReprojectMap */
} sg_map;

/*
 * The Ceres problem that Slam::SetupProblem builds (slam.cpp:257-414), in compact form.
 *   - one quaternion block (4, local 3 via ceres::QuaternionParameterization) + one translation block (3)
 *     per frame; a frame's blocks are free or constant independently (the translation of a skipped
 *     previous frame can be free through FrameDistance while its rotation is absent);
 *   - one homogeneous point block (4, no parameterization) per point, free or constant;
 *   - intrinsics blocks (7) per camera, constant unless cameras_free (SolveAllFrames(..., true));
 *   - residual blocks: ReprojectionError (2) with CauchyLoss(range) per observation, FrameDistance (1)
 *     with CauchyLoss(dist_range) per (frame, prev) pair, CameraStabilization (7) with CauchyLoss(5)
 *     per camera when cameras_free.
 */
typedef struct sg_problem {
  int32_t num_cameras;
  double* k;                    /* [7*ncam] */
  int32_t cameras_free;         /* 0: intrinsics constant (SolveFrames) */
  int32_t num_frames;
  double* q;                    /* [4*F] updated in place */
  double* t;                    /* [3*F] updated in place */
  int32_t* frame_camera;        /* [F] */
  uint8_t* frame_rot_free;      /* [F] */
  uint8_t* frame_trans_free;    /* [F] */
  int32_t* frame_map_index;     /* [F] source frame in the sg_map, or -1 */
  int32_t num_points;
  double* X;                    /* [4*P] updated in place */
  uint8_t* point_free;          /* [P] */
  int32_t* point_map_index;     /* [P] source point in the sg_map, or -1 */
  int32_t num_obs;
  double* obs_pt;               /* [2*M] observed pixel */
  int32_t* obs_frame;           /* [M] problem frame index */
  int32_t* obs_point;           /* [M] problem point index */
  int32_t num_dist;
  int32_t* dist_frame;          /* [D] FrameDistance(frame.t, prev.t) */
  int32_t* dist_prev;           /* [D] */
  double range;                 /* CauchyLoss(range) on reprojection (slam.cpp:265) */
  double dist_target;           /* FrameDistance(150.) (slam.cpp:403) */
  double dist_range;            /* CauchyLoss(15) (slam.cpp:404) */
  double stab_range;            /* CauchyLoss(5) on CameraStabilization (slam.cpp:463) */
  void* owner_;                 /* library-owned storage (sg_problem_from_map), NULL for caller-owned */
} sg_problem;

/* ceres::Solver::Options as used by Slam::Run (slam.cpp:482-508) plus the Ceres 1.8 defaults it keeps. */
typedef struct sg_solver_options {
  int32_t max_num_iterations;            /* 1000 (slam.cpp:493) */
  double function_tolerance;             /* 1e-7 (slam.cpp:494); 1e-9 when fine */
  double gradient_tolerance;             /* 1e-10, relative to the initial gradient max-norm (Ceres 1.8) */
  double parameter_tolerance;            /* 1e-8 */
  double min_relative_decrease;          /* 1e-3 */
  double initial_trust_region_radius;    /* 1e4 */
  double max_trust_region_radius;        /* 1e16 */
  double min_trust_region_radius;        /* 1e-32 */
  double min_lm_diagonal;                /* 1e-6 */
  double max_lm_diagonal;                /* 1e32 */
  int32_t max_num_consecutive_invalid_steps; /* 5 */
  int32_t jacobi_scaling;                /* 1 */
  int32_t disable_termination;           /* benchmark mode: run exactly max_num_iterations LM iterations */
  int32_t always_linearize;              /* benchmark mode: a rejected step re-linearizes too (same values),
                                            so every iteration is SURVEY.md 8d's full unit of work; 0 = Ceres */
} sg_solver_options;

/* ceres::Solver::Summary fields the reference reads (slam.cpp:510-520). */
typedef struct sg_solver_summary {
  int32_t num_iterations;        /* summary.iterations.size() — includes iteration 0 (slam.cpp:517) */
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int32_t num_invalid_steps;
  int32_t termination_type;      /* enum sg_termination */
  int32_t ok;                    /* summary.error.empty() (slam.cpp:520) */
  double initial_cost;           /* including fixed cost */
  double final_cost;             /* summary.final_cost (slam.cpp:518) */
  double fixed_cost;
  double trust_region_radius;
  int32_t num_lm_iterations;     /* LM loop iterations executed on the device (benchmark unit) */
  int32_t sync_timeouts;         /* Cholesky hand-off waits that hit their spin limit (0 in a healthy solve; a
                                    non-zero count ends the solve with SG_DEVICE_TIMEOUT) */
} sg_solver_summary;

typedef struct sg_device_options {
  int32_t device;                /* HIP device ordinal */
  int32_t precision;             /* 0: fp64 everywhere, the reference's arithmetic (the only mode: any other
                                    value is rejected with SG_EINVAL) */
  int32_t rank;                  /* landmark shard index (0 for single GPU) */
  int32_t nranks;                /* 1 for single GPU */
} sg_device_options;

/* ---------------------------------------------------------------------------------------------------- */
/* Library */
const char* sg_version(void);
const char* sg_last_error(void);              /* thread-local message for the last failing call */
void sg_solver_options_default(sg_solver_options* o);
void sg_device_options_default(sg_device_options* o);

/* ---------------------------------------------------------------------------------------------------- */
/* Problem assembly (host side of Slam::SetupProblem, slam.cpp:257-414 / SolveFrames 417-443 /
 * SolveAllFrames 447-480).  Returns 1 in *built when the problem was built, 0 when the reference aborts
 * ("Slam aborted due to frame set too small", slam.cpp:305-308). */
int sg_problem_from_map_frames(const sg_map* map, int32_t num_to_solve, int32_t num_to_present,
                               double range, sg_problem* out, int32_t* built);
int sg_problem_from_map_all(const sg_map* map, double range, int32_t solve_cameras,
                            sg_problem* out, int32_t* built);
void sg_problem_free(sg_problem* p);
/* Copy solved parameter blocks back into the map (what Ceres does through the raw pointers). */
int sg_problem_write_back(const sg_problem* p, sg_map* map);
/* Split a problem's landmarks into nranks shards (contiguous ranges of points sorted by first observing
 * frame); every shard keeps all frames, cameras and FrameDistance blocks. */
int sg_problem_shard(const sg_problem* p, int32_t rank, int32_t nranks, sg_problem* out);

/* ---------------------------------------------------------------------------------------------------- */
/* Device bundle-adjustment solver (Ceres 1.8 Levenberg-Marquardt + SPARSE_SCHUR, restated on MI355X). */
typedef struct sg_ba sg_ba;
int sg_ba_create(sg_ba** out, const sg_device_options* dev);
void sg_ba_destroy(sg_ba* h);
/* RCCL communicator for landmark sharding: id is ncclUniqueId (128 bytes), from sg_comm_unique_id. */
int sg_comm_unique_id(void* id128);
int sg_ba_comm_init(sg_ba* h, const void* id128, int32_t nranks, int32_t rank);
/* In-process communicator group: nranks (<= 8) solver handles on ONE device, each driven by its own host
 * thread, exchange through the group instead of RCCL (each all-reduce synchronises the rank's stream, meets
 * the others at a host barrier and sums in rank order).  Runs the landmark-sharded device chain (envelope
 * union, rank-0 assembly, packed S exchange, the replicated decision) on a one-GPU machine; for tests.
 * Destroy the group after every handle that uses it. */
typedef struct sg_comm_group sg_comm_group;
int sg_comm_group_create(sg_comm_group** out, int32_t nranks);
void sg_comm_group_destroy(sg_comm_group* g);
int sg_ba_comm_init_local(sg_ba* h, sg_comm_group* g, int32_t rank);
/* Host-callback communicator: one process per rank over any host collective (gloo, MPI).  Each of the solver's
 * all-reduces copies its device buffer to host memory, calls fn(buf, n, op, user) (op 0 = sum, 1 = max; return
 * 0 on success, nonzero fails the call with SG_ECOMM) and copies the result back — the call sequence of the
 * RCCL communicator (sg_ba_comm_init), with the transport on the host.  Must precede sg_ba_load. */
typedef int (*sg_allreduce_fn)(double* buf, long long n, int32_t op, void* user);
int sg_ba_comm_init_host(sg_ba* h, int32_t nranks, int32_t rank, sg_allreduce_fn fn, void* user);
/* Upload a problem (the problem's q/t/X are read now and written back by sg_ba_download). */
int sg_ba_load(sg_ba* h, const sg_problem* p);
/* Pre-size the handle's device and pinned staging buffers for problems of up to max_frames frames, max_points
 * points and max_obs observations (a map's high-water mark), so loads that follow do not reallocate on their
 * critical path.  Reallocation drops the loaded problem (load again).  The Slam facade does this itself,
 * reserving twice the largest window problem it has loaded. */
int sg_ba_reserve(sg_ba* h, int32_t max_frames, int32_t max_points, int32_t max_obs);
/* Incremental problem update (replaces the per-call rebuild of slam.cpp:257-414): a
 * load whose structure equals the previous load's (frames, cameras, freedom flags, observation incidence,
 * FrameDistance pairs) re-uploads the values only.  Counts of full and value-only loads on this handle. */
int sg_ba_load_counts(const sg_ba* h, int32_t* full_loads, int32_t* value_loads);
/* Run the LM solve on the device; writes the solved blocks back into p. */
int sg_ba_solve(sg_ba* h, const sg_solver_options* o, sg_problem* p, sg_solver_summary* s);
/* Benchmark entry: (re)initialise from the uploaded state, then enqueue exactly n LM iterations without
 * host synchronisation (termination disabled).  sg_ba_sync waits for completion. */
int sg_ba_begin(sg_ba* h, const sg_solver_options* o);
int sg_ba_iterate(sg_ba* h, int32_t n);
int sg_ba_sync(sg_ba* h);
int sg_ba_summary(sg_ba* h, sg_solver_summary* s);
int sg_ba_download(sg_ba* h, sg_problem* p);
/* Per-kernel timing over the last sg_ba_iterate calls (HIP events on the solver's stream). names is a
 * comma-separated list; ms[i] = mean duration of kernel i per launch; counts[i] launches timed. */
int sg_ba_set_timing(sg_ba* h, int32_t enable);
int sg_ba_kernel_times(sg_ba* h, char* names, int32_t names_len, double* ms, int32_t* counts, int32_t max);
/* Algorithmic byte / flop counts for the roofline (per launch of each timed kernel). */
int sg_ba_kernel_work(sg_ba* h, double* bytes, double* flops, int32_t max);

/* What the last sg_ba_load set up (diagnostics, benchmark records, shard balance). */
typedef struct sg_ba_info {
  int32_t num_frames, num_points, num_obs;   /* the loaded problem (this rank's landmark shard) */
  int32_t num_blocks;                        /* free camera blocks (frames with a free rotation or translation) */
  int32_t n;                                 /* reduced camera system dimension (6 blocks + free intrinsics) */
  int32_t band_tiles;                        /* widest row of the Cholesky envelope, in 16-wide tiles */
  int32_t cholesky_path;                     /* 0: tiled band (k_chol_tiles), 1: LDS window, 2: global memory
                                                (panel rows staged in LDS), 3: global memory, 4: bordered band
                                                (free intrinsics: frame band tiled, then the border) */
  int32_t num_pairs;                         /* Schur observation pairs (s <= t) of this rank's free points */
  int32_t rank, nranks;
  int32_t cholesky_split;                    /* tiled path: tile rows factored bottom-up by a second workgroup
                                                (dissected band; 0: one workgroup) */
  int32_t num_allreduces;                    /* landmark-shard sum all-reduces this handle has issued in LM
                                                iterations (0 on one rank) */
  int32_t lin_waves;                         /* waves per Jacobian-sweep chunk (1, or 2 when the doubled grid
                                                fits the device at once) */
  int32_t cholesky_separator;                /* tiled path with a split: the separator's tile rows (<= 7) */
  int32_t cholesky_stile;                    /* tiled path: the last LM iteration enqueued loaded its tiles from the
                                                tile-major copy of the band that the S reduce writes (1), or from
                                                row-major S (0: landmark shards, packed S, SG_CHOL_STILE=0) */
  int32_t wt_stores;                         /* launch outputs stored write-through: bit 0 the Jacobian records,
                                                bit 1 the camera partials, bit 2 the Schur slabs (SG_WT_STORES) */
} sg_ba_info;
int sg_ba_info_get(const sg_ba* h, sg_ba_info* out);

/* Jacobian/Hessian sweep only (benchmark of the HBM-bound kernel): n linearizations at the current
 * state (k_linearize + camera-block reduce), timed when sg_ba_set_timing is on. */
int sg_ba_sweep(sg_ba* h, int32_t n);

/* Residual sweep only (ReprojectionError over the uploaded observations at the current state):
 * r[2*M] corrected residuals in problem order, returns cost (without fixed cost) and failure count. */
int sg_ba_evaluate(sg_ba* h, double* residuals, double* cost, int32_t* num_failed);

/* ---------------------------------------------------------------------------------------------------- */
/* Slam facade (slam.h:21-65).  A handle keeps iterations()/error() like the reference's Slam object. */
typedef struct sg_slam sg_slam;
int sg_slam_create(sg_slam** out, const sg_device_options* dev);
void sg_slam_destroy(sg_slam* s);
int sg_slam_solve_frames(sg_slam* s, sg_map* map, int32_t num_to_solve, int32_t num_to_present,
                         double range, int32_t* solved);                          /* slam.cpp:417-443 */
int sg_slam_solve_all_frames(sg_slam* s, sg_map* map, double range, int32_t solve_cameras,
                             int32_t* solved);                                    /* slam.cpp:447-480 */
int sg_slam_reproject_map(sg_slam* s, sg_map* map, double* mean);               /* slam.cpp:523-548 */
int32_t sg_slam_iterations(const sg_slam* s);                                    /* slam.h:49 */
double sg_slam_error(const sg_slam* s);                                          /* slam.h:50 */
int sg_slam_load_counts(const sg_slam* s, int32_t* full_loads, int32_t* value_loads);   /* see sg_ba_load_counts */
/* Host wall time (ms) of the last SolveFrames / SolveAllFrames call by phase: [0] SetupProblem (problem build),
 * [1] sg_ba_load (work lists + upload), [2] device LM loop incl. download, [3] write-back into the map.
 * A development aid for sizing the host share of a real call (tools/e2e_replay.py). */
int sg_slam_last_phase_ms(const sg_slam* s, double* ms4);
int sg_slam_last_summary(const sg_slam* s, sg_solver_summary* out);
/* Pose-only (motion-only) bundle adjustment: given the landmarks as they are, where are these frames?  It fills
 * the place of Slam::SolveFramePose (slam.h:21-65; the reference disabled its body, slam.cpp:180-182, and calls it
 * as Matcher::Track's update_frames hook, main.cpp:560-563).  For each listed frame f, solved on its own against
 * the map as it is at entry, the problem Slam::SetupProblem (slam.cpp:257-414) would build if only f were free:
 * one ReprojectionError with CauchyLoss(range) per observation of f that is not disabled and whose point is
 * slam-usable (slam.cpp:280-283); q_f free with ceres::QuaternionParameterization (slam.cpp:312-313), t_f free,
 * every point and the intrinsics constant; with_frame_distance and frame_prev[f] >= 0 add FrameDistance(150) with
 * CauchyLoss(15) to the previous frame's constant translation (slam.cpp:86-105, 401-410).  The solver is the
 * handle's sg_solver_options (sg_slam_set_options) on the Ceres 1.8 LM of sg_ba_solve; all frames of a call run in
 * one device launch, one workgroup each.
 *   - A frame with fewer than 3 usable observations is not solved: solved[i] = 0, SG_DID_NOT_RUN, pose untouched.
 *   - A frame whose solve ends with ok = 0 (a start behind the camera: SG_NUMERICAL_FAILURE) also keeps its pose
 *     and gets solved[i] = 0.  Otherwise q_f and t_f are written into the map; nothing else of the map is.
 *   - A frame index out of range or listed twice: SG_EINVAL, nothing changed.  n == 0 returns SG_OK before the
 *     handle or the device is touched.
 * summaries (may be NULL) receives each frame's summary.  As Slam::Run does for any solve (slam.cpp:517-518),
 * sg_slam_iterations grows by the num_iterations of the frames that ran, and sg_slam_error / sg_slam_last_summary
 * take the values of the last listed frame that ran.  No communicator is involved: rank-local on a sharded handle. */
int sg_slam_solve_frame_poses(sg_slam* s, sg_map* map, const int32_t* frames, int32_t n, double range,
                              int32_t with_frame_distance, int32_t* solved /*[n]*/,
                              sg_solver_summary* summaries /*[n], may be NULL*/);
/* Structure-only bundle adjustment, the dual of sg_slam_solve_frame_poses: given the frames as they are, where
 * are these landmarks?  Its first customers are the points Matcher::Track seeds at a guessed depth
 * (Unproject(..., 2000), localmap.cpp:106-110), which the window solve does not touch while they carry
 * NO_BASELINE | NO_OBSERVATIONS.  Each listed point p is solved on its own against the map as it is at entry:
 *   - Residuals: one ReprojectionError (slam.cpp:60-84, 285-294) with CauchyLoss(range) per observation of p with
 *     obs_disabled == 0, in map order, from whatever frame.
 *   - Point flags are NOT consulted and not written.  This differs from Slam::SetupProblem's filter (slam.cpp:280-283
 *     skips every point that is not slam-usable): the caller runs Clean / CheckFlags afterwards as before.
 *   - Parameter blocks: X[4p .. 4p+3] free without a parameterization (4 unknowns, as slam.cpp leaves it); every
 *     frame and every intrinsics block constant; no FrameDistance; fixed_cost is 0.
 *   - Solver: the handle's sg_solver_options (sg_slam_set_options) on the Ceres 1.8 LM of sg_ba_solve: Jacobi
 *     scaling, the clamped LM diagonal, a 4x4 Cholesky of the damped scaled system (a non-positive pivot makes an
 *     invalid step), the model cost change from the stored system, the same step decision.  Every point has its
 *     own trust region.  All points of a call run in one device launch, eight lanes each.
 *   - A point with fewer than 2 enabled observations is not solved: solved[i] = 0, SG_DID_NOT_RUN, X untouched
 *     (decided before anything is launched).
 *   - A point whose solve ends with ok = 0 (a start behind one of its cameras, or
 *     max_num_consecutive_invalid_steps invalid steps in a row: SG_NUMERICAL_FAILURE) also keeps its X and gets
 *     solved[i] = 0.  Otherwise the four doubles are written as the solver leaves them, not renormalized (as Ceres
 *     does through the raw pointer); nothing else of the map is written.
 *   - A point index out of range or listed twice: SG_EINVAL, nothing changed.  n < 0 or a null s or map:
 *     SG_EINVAL.  n == 0 returns SG_OK before the handle or the device is touched.
 * summaries (may be NULL) receives each point's summary.  sg_slam_iterations grows by the num_iterations of the
 * points that ran, and sg_slam_error / sg_slam_last_summary take the values of the last listed point that ran (the
 * convention of sg_slam_solve_frame_poses).  No communicator is involved: rank-local on a sharded handle. */
int sg_slam_solve_points(sg_slam* s, sg_map* map, const int32_t* points, int32_t n, double range,
                         int32_t* solved /*[n]*/, sg_solver_summary* summaries /*[n], may be NULL*/);

/* Linear multi-view triangulation: given the frames as they are, where are these landmarks, from their
 * observations alone?  ("Triangulate points for initialization after there are known poses", main.cpp:3.)  Unlike
 * sg_slam_solve_points it needs no start: the location at entry is not read, so a point seeded at a guessed depth
 * (Unproject(..., 2000)), or one whose start projects behind a camera, gets the closed-form answer.  Per listed
 * point, from its observations with obs_disabled == 0, in map order, from whatever frame (point flags are not
 * consulted and not written):
 *   1. each pixel is undistorted to plane coordinates (a, b) by Newton on the radius (the inverse of
 *      Camera::PlaneToPixel, localmap.h:38-56, to rounding; not PixelToPlane's three fixed-point rounds);
 *   2. a local frame for conditioning: origin c0 = the first observation's camera centre, unit L = the rms distance
 *      of the observing centres from c0.  L == 0: SG_TRI_NO_BASELINE;
 *   3. two rows [n, -n . c_i] per observation, n = a r3 - r1 and n = b r3 - r2 (r1..r3 the rows of the frame's
 *      rotation, c_i = (t_i - c0) / L), summed into the symmetric 4x4 M;
 *   4. y = the unit eigenvector of M's smallest eigenvalue (cyclic Jacobi), eigenvalues l0 <= l1 <= l2 <= l3.
 *      l1 - l0 <= 1e-12 l3, or any non-finite value: SG_TRI_DEGENERATE;
 *   5. X = (L y.xyz + c0 y.w, y.w), with the sign that makes X.w >= 0 (X.w == 0: the sign that puts the point in
 *      front of the first observation's camera), scaled to unit 4-norm as Frame::Unproject leaves it
 *      (localmap.cpp:35).  The reference's own behind-camera test p.z < 0.001 X.w (project.h:27) accepts a point
 *      behind every camera when W < 0, both sides being negative; with W >= 0 fixed first it is the physical test;
 *   6. at X: behind = the observations the projection rejects (project.h:27), max_error_px = the largest
 *      reprojection error of the others, parallax = the largest angle at the point between the directions to an
 *      observing centre and to the first one;
 *   7. the status is the first of sg_tri_status' rules that applies, in the order of the enum below.
 * solved[i] = 1 and X is written for exactly the SG_TRI_OK points; every other point keeps its X.  With refine != 0
 * the SG_TRI_OK points are then polished by sg_slam_solve_points' solver (the handle's sg_solver_options,
 * CauchyLoss(range)) from the triangulated location, on the device, without a host round trip: the written X is
 * that solve's when it ends with ok = 1 and the triangulated one otherwise (solved[i] stays 1).  Nothing else of
 * the map is written, and a failing call writes nothing.
 *   - A point index out of range or listed twice: SG_EINVAL.  n < 0 or a null s, map or options: SG_EINVAL.
 *     n == 0 returns SG_OK before the handle or the device is touched.
 * results (may be NULL) receives each point's sg_triangulate_result, summaries (may be NULL) the polish's summary
 * (SG_DID_NOT_RUN for every point the polish did not run on).  sg_slam_iterations, sg_slam_error and
 * sg_slam_last_summary move only by the polish, by the convention of sg_slam_solve_points. */
enum sg_tri_status {
  SG_TRI_OK = 0,
  SG_TRI_DID_NOT_RUN = 1,    /* fewer than 2 enabled observations (decided before anything is launched) */
  SG_TRI_NO_BASELINE = 2,    /* every observation from one camera centre */
  SG_TRI_DEGENERATE = 3,     /* the null direction of M is not determined, or a non-finite value */
  SG_TRI_BEHIND = 4,         /* behind at least one of its cameras */
  SG_TRI_LOW_PARALLAX = 5,   /* parallax < min_parallax */
  SG_TRI_HIGH_ERROR = 6      /* max_error_px > the max_error_px option */
};

typedef struct sg_triangulate_options {
  double min_parallax;   /* rad; 0 = no gate */
  double max_error_px;   /* px;  0 = no gate */
  int32_t refine;        /* != 0: k_point_lm from the triangulated location */
  double range;          /* CauchyLoss range of the polish (ignored when refine == 0) */
} sg_triangulate_options;

typedef struct sg_triangulate_result {
  int32_t status, num_obs;                  /* enum sg_tri_status; enabled observations */
  double parallax, max_error_px, rel_gap;   /* rad; px; (l1 - l0) / l3 */
  double X[4];                              /* triangulated location (before the polish); zeros unless computed */
} sg_triangulate_result;

void sg_triangulate_options_default(sg_triangulate_options* o);   /* gates off, refine = 0, range = 2.0 */
int sg_slam_triangulate_points(sg_slam* s, sg_map* map, const int32_t* points, int32_t n,
                               const sg_triangulate_options* options, int32_t* solved /*[n]*/,
                               sg_triangulate_result* results /*[n], may be NULL*/,
                               sg_solver_summary* summaries /*[n], may be NULL*/);

/* Localization from scratch: given the points as they are, where is this frame, from its observations alone?
 * sg_slam_solve_frame_poses needs a start inside the basin (the reference starts a new frame at the pose of two
 * frames ago, main.cpp:540-552) and its Cauchy loss copes with a few bad correspondences, not with half of them;
 * after a tracking loss, a fast turn or a revisit ("Consider loop closing when adding new points", main.cpp:10)
 * nothing else here recovers.  This call does: P3P RANSAC on the device, then optionally that solver as the polish.
 * The pose at entry is not read.  Per listed frame f, over the records of sg_slam_solve_frame_poses (observations
 * with obs_disabled == 0 whose point is slam-usable, in map order; N of them), with no FrameDistance term:
 *   1. Run rule: N < 4: SG_LOC_DID_NOT_RUN (decided before anything is launched).
 *   2. Hypotheses: H = max_hypotheses rounded up to a multiple of 256 (anything above 2^20 is taken as 2^20).
 *      Hypothesis h in [0, H) draws three distinct record indices from a counter-based hash of (seed, f, h), f being
 *      the map's frame index (not the position in the list), with no state carried between hypotheses.  On 32-bit
 *      unsigned arithmetic:
 *          mix(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *          base = mix(mix(mix(seed) + f) + h);   r_j = mix(base ^ (0x9e3779b9 * (j + 1))),  j = 0, 1, 2
 *          i0 = (r_0 * N) >> 32,  i1 = (r_1 * (N - 1)) >> 32,  i2 = (r_2 * (N - 2)) >> 32   (64-bit products)
 *          if i1 >= i0: i1 += 1;   lo = min(i0, i1), hi = max(i0, i1);   if i2 >= lo: i2 += 1;  if i2 >= hi: i2 += 1
 *      (csrc/pnp_math.h, PnpSample).  A sample containing a point with |X.w| < 1e-9 (X has unit 4-norm: a point
 *      farther than 1e9 map units) yields no model; so does one with two equal bearings or three collinear points
 *      (squared sine below 1e-20), and one whose P3P has no finite real solution.
 *   3. Minimal solver, in fp64: the three pixels are undistorted to unit bearings (Newton on the radius, as in
 *      sg_slam_triangulate_points), the points are X.xyz / X.w.  Grunert's P3P: a quartic in the ratio of two depths,
 *      solved in closed form (Ferrari), up to four real roots in a fixed order (the position is the "root index");
 *      each root's depths take three Newton steps on the three distance equations; the rotation comes from the
 *      orthonormal triads of the two congruent triangles.  Poses are in the map's convention: p = q (X - t), Eigen
 *      [x,y,z,w] memory, t the camera centre, unit q with q.w >= 0.
 *   4. Scoring: every pose against all N records with the projection of sg_ba_evaluate (project.h:11-54, its
 *      behind-camera rule included).  MSAC cost = sum over the records of min(e^2, tau^2), e the pixel error,
 *      tau = threshold_px; a record the projection refuses counts tau^2.  It is formed as T tau^2 + s: T the
 *      truncated records, s the sum of e^2 over the others in index order.  The winner has the smallest cost (as a
 *      double).  Ties go to the pose with more inliers, then to the smaller s (on clean data with outliers present
 *      every all-inlier sample's s vanishes in the rounding of T tau^2 + s; this keeps the most accurate of them,
 *      not the first), then to the smaller h, then to the smaller root index.
 *   5. Status: the first of sg_loc_status' rules that applies, in the order of the enum below.  An inlier is a
 *      record with e^2 <= tau^2.
 *   6. Polish (refine != 0, SG_LOC_OK frames): sg_slam_solve_frame_poses' solver on all N records with
 *      CauchyLoss(range) and the handle's sg_solver_options, started at the winner, on the device without a host
 *      round trip.  The written pose is the polish's when it ends with ok = 1 and its MSAC cost at tau is not larger
 *      than the winner's (both from the same fixed-order reduction, ties as in step 4); otherwise the winner is
 *      written and refined = 0.
 *   7. solved[i] = 1 and q, t are written for exactly the SG_LOC_OK frames.  Nothing else of the map is written, and
 *      a failing call writes nothing.
 *   - A null s, map or options, n < 0, threshold_px <= 0 (or NaN), max_hypotheses <= 0, a frame index out of range
 *     or listed twice: SG_EINVAL.  n == 0 returns SG_OK before the handle or the device is touched.
 * results (may be NULL) receives each frame's sg_localize_result; obs_inlier (may be NULL, [map->num_obs]) 1 or 0
 * for each record of an SG_LOC_OK frame, at the written pose, and -1 everywhere else; summaries (may be NULL) the
 * polish's summary (SG_DID_NOT_RUN where it did not run).  sg_slam_iterations, sg_slam_error and
 * sg_slam_last_summary move only by the polish, by the convention of sg_slam_solve_frame_poses.  No communicator is
 * involved: rank-local on a sharded handle.
 * Not in scope: adaptive early termination (the hypothesis count is fixed, which keeps results reproducible),
 * degenerate-configuration tests beyond the ones of step 2, the FrameDistance term, any change to obs_disabled. */
enum sg_loc_status {
  SG_LOC_OK = 0,
  SG_LOC_DID_NOT_RUN = 1,   /* fewer than 4 records (decided before anything is launched) */
  SG_LOC_NO_MODEL = 2,      /* no hypothesis gave a finite pose */
  SG_LOC_FEW_INLIERS = 3    /* the winner has fewer than max(min_inliers, 4) inliers */
};

typedef struct sg_localize_options {
  double threshold_px;      /* tau: inlier threshold and MSAC truncation, px; > 0 */
  int32_t max_hypotheses;   /* > 0; rounded up to a multiple of 256 */
  int32_t min_inliers;      /* fewer inliers at the winner: SG_LOC_FEW_INLIERS (at least 4 are always required) */
  uint32_t seed;
  int32_t refine;           /* != 0: k_pose_lm from the winner */
  double range;             /* CauchyLoss range of the polish (ignored when refine == 0) */
} sg_localize_options;

typedef struct sg_localize_result {
  int32_t status, num_obs;           /* enum sg_loc_status; records N */
  int32_t num_inliers, refined;      /* inliers at the written pose; 1: the written pose is the polish's */
  int32_t best_hypothesis;           /* the winner's h; -1 without a model */
  int32_t best_sample[3];            /* its record indices within the frame, in draw order; -1 without a model */
  int32_t hypotheses, models;        /* H; hypotheses that produced at least one pose */
  double msac_cost, inlier_rms_px;   /* at the written pose (the winner's when the frame is not SG_LOC_OK) */
  double ransac_cost;                /* the winner's MSAC cost */
  double q[4], t[3];                 /* the RANSAC winner, before the polish; zeros without a model */
} sg_localize_result;

void sg_localize_options_default(sg_localize_options* o);   /* 4.0, 1024, 8, seed 0, refine = 1, range = 2.0 */
int sg_slam_localize_frames(sg_slam* s, sg_map* map, const int32_t* frames, int32_t n,
                            const sg_localize_options* options, int32_t* solved /*[n]*/,
                            sg_localize_result* results /*[n], may be NULL*/,
                            int32_t* obs_inlier /*[map->num_obs], may be NULL*/,
                            sg_solver_summary* summaries /*[n], may be NULL*/);

/* Relative pose of frame pairs: where is frame b relative to frame a, from the pixels they share alone?  Every call
 * above needs the other half of the map; this one starts a map, or re-joins two frames that share no trusted
 * landmark.  (The reference never solves this: it starts a frame at the pose of two frames ago, assumes the 150 mm
 * stereo baseline, main.cpp:496, 540-552, and seeds points at a guessed depth; ApplyEpipolarConstraint only checks
 * an essential matrix built from poses that exist.)  8-point RANSAC on the device, all listed pairs (a, b) in one
 * call, pairs[2i] = a, pairs[2i + 1] = b:
 *   1. Records: the points with an observation with obs_disabled == 0 in a and one in b, in the map order of a's
 *      observations; where a frame has several enabled observations of the point, the first.  Point flags, point
 *      locations and both poses are not consulted.  A record is four doubles, the pixel in a then the pixel in b.
 *      N < 8: SG_REL_DID_NOT_RUN, decided on the host before anything is launched.
 *   2. Hypotheses: H = max_hypotheses rounded up to a multiple of 256 (anything above 2^20 is taken as 2^20).
 *      Hypothesis h draws eight distinct record indices, sg_slam_localize_frames' scheme extended: with
 *      key = a * 65536 + b (map frame indices), base = mix(mix(mix(seed) + key) + h), r_j = mix(base ^ (0x9e3779b9 *
 *      (j + 1))), i_j = (r_j * (N - j)) >> 32 for j = 0 .. 7, and each i_j is then stepped over the earlier indices
 *      taken in ascending order (i_j >= p: i_j += 1).  Nothing is carried between hypotheses (csrc/relpose_math.h,
 *      RelSample).
 *   3. Minimal solver, fp64: both pixels of each sampled record are undistorted to plane coordinates (Newton on the
 *      radius, as in sg_slam_triangulate_points); each side gets Hartley's normalisation (centroid to the origin, rms
 *      distance sqrt 2); the eight epipolar rows x_b' (x) x_a' are summed into the symmetric 9x9 moment matrix M; e is
 *      the unit eigenvector of its smallest eigenvalue; the 3x3 is de-normalised and projected to singular values
 *      (1, 1, 0) (EssentialFromMoments).  The eigenvector: L D L^T of M + 2^-40 tr(M) I without pivoting, inverse
 *      iteration from a fixed start until two iterates agree to 1e-15 in every entry (40 rounds at the most).  l0 and
 *      l1 come from that iteration and a second, deflated one, l8 from 16 power iterations.  A sample gives no model
 *      when a value is not finite, a pivot is not positive, the iteration has not converged, or the null direction is
 *      not determined: (l1 - l0) / l8 <= 1e-12.
 *   4. Scoring: every E against all N records by the squared Sampson distance in ideal pixels, F = K_b^-T E K_a^-1 on
 *      the undistorted pixels (fx x + cx, fy y + cy).  MSAC cost = sum of min(e^2, tau^2), formed as T tau^2 + s: T
 *      the truncated records (a non-finite e^2 counts as truncated), s the sum of e^2 over the others in index order.
 *      The winner and every tie-break are sg_slam_localize_frames' (step 4 there); the root index is always 0.
 *      The hypotheses are ranked by that index-order sum.  The figures reported for the winner and compared in step
 *      6 (msac_cost, ransac_cost, inlier_rms_px) come from a fixed-order workgroup reduction instead: thread t of
 *      256 sums records t, t + 256, ... in index order, then the 64 lanes of a wave and the four waves are summed
 *      in a fixed order.  They are reproducible bit for bit and can differ from the index-order sum in the last bits.
 *   5. Pose: the four decompositions (R1, +u3), (R1, -u3), (R2, +u3), (R2, -u3) of the winner (R1 = U W V^T,
 *      R2 = U W^T V^T, det +1) are each tested on its inliers: the two depths of d_b f_b = d_a R f_a + t by the 2x2
 *      least squares of the bearings f = (x, y, 1); a record is in front when both are positive.  The most in-front
 *      inliers win, ties to the earlier.  Output in the map's convention p = q (X - t): q_rel with
 *      p_b = q_rel (p_a - t_rel), unit, w >= 0, Eigen memory; t_rel the centre of b in a's camera coordinates, of unit
 *      length (scale is not observable).  A record's parallax is the angle between R f_a and f_b.  E is reported
 *      with the sign that makes it [t]x R of that decomposition (t = -R t_rel).
 *   6. Local optimisation (refine != 0, at most two rounds): EssentialFromMoments on the moments of all current
 *      inliers (normalised over them), summed by a fixed-order workgroup reduction; all N records are re-scored; the
 *      result is kept only when its MSAC key is not after the current one in step 4's order (the second round is
 *      skipped when the first was not kept).  refined reports the rounds kept.  Fewer than 8 inliers: no round.
 *   7. Status: the first of sg_rel_status' rules that applies, in the order of the enum below.
 *   8. solved[i] = 1 exactly for SG_REL_OK.  With baseline > 0, frame b of an OK pair is written from frame a's pose
 *      as it was at entry: q_b = q_rel (x) q_a renormalised with w >= 0, t_b = t_a + baseline R_a^T t_rel; nothing
 *      else of the map is written.  With baseline == 0 the map is not written.  A failing call writes nothing.
 *   - SG_EINVAL: a null s, map or options; n < 0; threshold_px <= 0 or NaN; max_hypotheses <= 0; baseline < 0 or NaN;
 *     a frame index out of range; a == b; the same b listed twice; frames on cameras whose intrinsics cannot both be
 *     read (frame_camera out of range, or no k); record arrays asked for with rec_capacity below the call's records.
 *     All of these are found on the host before the device is touched.  n == 0 returns SG_OK before the handle or
 *     the device is touched.
 * results (may be NULL) receives each pair's sg_relpose_result.  rec_offset (may be NULL, [n + 1]) receives the
 * pairs' record ranges; rec_inlier (may be NULL, [rec_capacity]) per record 1 or 0 for OK pairs and -1 elsewhere;
 * rec_obs (may be NULL, [2 rec_capacity]) per record its map observation index in a, then in b, so that a caller can
 * disable the outliers.  The call's records never exceed the sum over the pairs of a's observations.
 * sg_slam_iterations, sg_slam_error and sg_slam_last_summary do not move.  No communicator is involved: rank-local.
 * Not in scope: the 5-point solver; planar or homography model selection (the 8-point is degenerate when every record
 * lies on one plane: such a pair gives SG_REL_NO_MODEL or an unreliable pose); a non-linear 5-DoF polish; adaptive
 * termination; any change to obs_disabled. */
enum sg_rel_status {
  SG_REL_OK = 0,
  SG_REL_DID_NOT_RUN = 1,     /* fewer than 8 records (decided before anything is launched) */
  SG_REL_NO_MODEL = 2,        /* no hypothesis gave an essential matrix */
  SG_REL_FEW_INLIERS = 3,     /* fewer than max(min_inliers, 8) inliers */
  SG_REL_NO_CHEIRALITY = 4,   /* the best decomposition has fewer than max(min_inliers, 8) in-front inliers */
  SG_REL_LOW_PARALLAX = 5     /* min_parallax > 0 and fewer than max(min_inliers, 8) in-front inliers with
                                 parallax >= min_parallax: the pure-rotation guard */
};

typedef struct sg_relpose_options {
  double threshold_px;      /* tau: inlier threshold and MSAC truncation, ideal px; > 0 */
  int32_t max_hypotheses;   /* > 0; rounded up to a multiple of 256 */
  int32_t min_inliers;
  double min_parallax;      /* rad; 0 = no gate */
  uint32_t seed;
  int32_t refine;           /* != 0: local optimisation */
  double baseline;          /* > 0: write frame b at this distance from a; 0: do not write the map */
} sg_relpose_options;

typedef struct sg_relpose_result {
  int32_t status, num_obs;               /* enum sg_rel_status; records N */
  int32_t num_inliers, num_front, num_parallax, refined;
  int32_t best_hypothesis;               /* the winner's h; -1 without a model */
  int32_t best_sample[8];                /* its record indices within the pair, in draw order; -1 without a model */
  int32_t hypotheses, models;            /* H; hypotheses that produced a model */
  double msac_cost, ransac_cost;         /* at the reported E; at the RANSAC winner */
  double inlier_rms_px;
  double q[4], t[3], E[9];               /* q_rel, t_rel; E row-major, Frobenius norm sqrt 2; zeros without a model */
} sg_relpose_result;

void sg_relpose_options_default(sg_relpose_options* o);   /* 2.0, 1024, 16, 0, seed 0, refine = 1, baseline = 0 */
int sg_slam_relative_poses(sg_slam* s, sg_map* map, const int32_t* pairs /*[2n]*/, int32_t n,
                           const sg_relpose_options* options, int32_t* solved /*[n]*/,
                           sg_relpose_result* results /*[n], may be NULL*/, int32_t* rec_offset /*[n+1], may be NULL*/,
                           int32_t* rec_inlier /*[rec_capacity], may be NULL*/,
                           int32_t* rec_obs /*[2 rec_capacity], may be NULL*/, int32_t rec_capacity);

/* Alignment of matched landmarks: which similarity joins two pieces of one map?  After a revisit ("Consider loop
 * closing when adding new points", main.cpp:5), or when a map restarted with sg_slam_relative_poses has to be put back
 * into the old one, the same landmarks stand twice in one sg_map, in two coordinate systems that differ by a rotation,
 * a translation and a scale (a monocular restart has no scale; a long stereo run drifts).  The Hamming matcher
 * delivers the landmark-to-landmark matches, wrong pairs included; this call turns them into the transform
 * Y = scale R(q) X + t from the a side to the b side, by 3-point Sim(3) RANSAC on the device, and
 * sg_map_apply_similarity applies it.  All groups of a call run in two launches.  Per group g, over the
 * correspondences corr[2 j], corr[2 j + 1] (point a, point b; map point indices), j in
 * [group_offset[g], group_offset[g + 1]):
 *   1. Records: a correspondence becomes a record when both points are slam-usable (none of the flags BAD_LOCATION,
 *      NO_BASELINE, NO_OBSERVATIONS, BAD_FEATURE, the filter of sg_slam_solve_frame_poses), all eight doubles of the two
 *      locations are finite and |W| >= 1e-9 |X|_2 on both sides.  A record is six doubles, X_a.xyz / X_a.w then
 *      X_b.xyz / X_b.w, in listed order; N of them.  N < 4: SG_ALIGN_DID_NOT_RUN, decided on the host before anything is
 *      launched.  The map's frames, observations and pixels are not read.
 *   2. Hypotheses: H = max_hypotheses rounded up to a multiple of 256 (anything above 2^20 is taken as 2^20).
 *      Hypothesis h draws three distinct record indices exactly as in sg_slam_localize_frames step 2 (PnpSample), with
 *      the map index of point a of the group's first listed correspondence in the place of the frame index: the
 *      result does not depend on the group's position in the call.
 *   3. Minimal solver, fp64, Horn's closed form (csrc/align_math.h); the same function serves three records and all
 *      inliers.  Centroids xm, ym, centred x', y', S_ab = sum x'_a y'_b; the symmetric 4x4 N in (w, x, y, z) order
 *          row 0:      Sxx+Syy+Szz, Syz-Szy, Szx-Sxz, Sxy-Syx
 *          diagonal:   Sxx-Syy-Szz, -Sxx+Syy-Szz, -Sxx-Syy+Szz
 *          the rest:   N12 = Sxy+Syx, N13 = Szx+Sxz, N23 = Syz+Szy;
 *      q is the unit eigenvector of N's largest eigenvalue l3 (cyclic Jacobi, sg_slam_triangulate_points' TriJacobi4,
 *      on -N); gap = (l3 - l2) / l3 with l2 the next eigenvalue, which is 2 (s2 + s3) / (s1 + s2 + s3) in the singular
 *      values of S for a proper match: 0 for collinear points, of order one for a spread set.
 *      scale = sqrt(sum |y'|^2 / sum |x'|^2), or 1 with fix_scale; t = ym - scale R xm.  No model when a value is not
 *      finite, sum |x'|^2 or sum |y'|^2 is 0, l3 <= 0, gap <= 1e-12, or scale is outside [1 / max_scale, max_scale]
 *      (max_scale == 0: no gate).
 *   4. Scoring: e^2 = |Y - (scale R X + t)|^2, in b's coordinates, against all N records.  MSAC cost = sum of
 *      min(e^2, tau^2), tau = threshold, formed as T tau^2 + s exactly as in sg_slam_localize_frames step 4: T the
 *      truncated records (a non-finite e^2 counts as truncated), s the sum of e^2 over the others in index order.  The
 *      winner and every tie-break are that step's (more inliers, then the smaller s, then the smaller h); the root
 *      index is always 0.  The hypotheses are ranked by the index-order sum; the figures reported for the winner and
 *      compared in step 5 (msac_cost, ransac_cost, inlier_rms) come from the fixed-order workgroup reduction of
 *      sg_slam_relative_poses step 4 (thread t of 256 sums records t, t + 256, ..., then the lanes and the waves in a
 *      fixed order): reproducible bit for bit, and they can differ from the index-order sum in the last bits.
 *   5. Local optimisation (refine != 0, at most two rounds, needs at least 4 inliers): step 3 on all current inliers
 *      (e^2 <= tau^2), by two fixed-order workgroup reductions, the centroids first and then the centred moments
 *      (never raw second moments: map coordinates are thousands of units against spreads of hundreds); all N records
 *      are re-scored; the result is kept only when its MSAC key is not after the current one in step 4's order (the
 *      second round is skipped when the first was not kept).  refined reports the rounds kept.
 *   6. Status: the first of sg_align_status' rules that applies, in the order of the enum below.  gap is always that
 *      of the N matrix of the final inliers (those of the reported transform), with refine == 0 too, and 0 where that
 *      matrix gives no finite value; gap < min_gap: SG_ALIGN_DEGENERATE (the inliers are collinear to that degree and
 *      do not fix the rotation about their line).
 *   7. solved[g] = 1 exactly for SG_ALIGN_OK.  corr_inlier (may be NULL, one int per correspondence of the call) is 1
 *      or 0 for each record of an OK group at the reported transform, and -1 for correspondences that are no records
 *      and for groups that are not OK.  The map is never written by this call; sg_slam_iterations, sg_slam_error and
 *      sg_slam_last_summary do not move.  No communicator is involved: rank-local on a sharded handle.
 *   - SG_EINVAL, all found on the host before the device is touched: a null s, map or options; n < 0; with n > 0 a null
 *     group_offset or solved, and a null corr when the call lists a correspondence; group_offset[0] != 0 or a
 *     decreasing offset; a point index out of range; a correspondence with a == b; threshold <= 0 or NaN;
 *     max_hypotheses <= 0; min_gap < 0 or NaN; max_scale neither 0 nor >= 1.  n == 0 returns SG_OK before the handle or
 *     the device is touched.  A failing call writes nothing.
 * results (may be NULL) receives each group's sg_align_result.
 * Not in scope: scoring by reprojection in the frames or depth-weighted thresholds; adaptive termination; merging the
 * duplicated landmarks or their observations; any change to obs_disabled or point flags. */
enum sg_align_status {
  SG_ALIGN_OK = 0,
  SG_ALIGN_DID_NOT_RUN = 1,   /* fewer than 4 records (decided on the host, before any launch) */
  SG_ALIGN_NO_MODEL = 2,      /* no hypothesis gave a finite transform inside the scale gate */
  SG_ALIGN_FEW_INLIERS = 3,   /* fewer than max(min_inliers, 4) inliers */
  SG_ALIGN_DEGENERATE = 4     /* the inliers do not fix the rotation: gap < min_gap (collinear landmarks) */
};

typedef struct sg_align_options {
  double threshold;         /* tau: inlier threshold and MSAC truncation, map units; > 0 */
  int32_t max_hypotheses;   /* > 0; rounded up to a multiple of 256 */
  int32_t min_inliers;
  uint32_t seed;
  int32_t refine;           /* != 0: local optimisation, at most two rounds */
  int32_t fix_scale;        /* != 0: scale = 1 (rigid alignment, for maps whose scale the stereo baseline fixes) */
  double max_scale;         /* 0: no gate; otherwise >= 1: a transform with scale outside [1 / max_scale, max_scale]
                               is no model */
  double min_gap;           /* >= 0 */
} sg_align_options;

typedef struct sg_align_result {
  int32_t status, num_corr, num_records, num_inliers, refined;   /* enum sg_align_status; listed; records N */
  int32_t best_hypothesis, best_sample[3];   /* the winner's h and record indices in draw order; -1 without a model */
  int32_t hypotheses, models;                /* H; hypotheses that produced a model */
  double msac_cost, ransac_cost, inlier_rms, gap;   /* at the reported transform; at the RANSAC winner */
  double scale, q[4], t[3];   /* Y = scale R(q) X + t; q unit, Eigen [x,y,z,w], w >= 0; zeros without a model */
} sg_align_result;

void sg_align_options_default(sg_align_options* o);   /* 10.0, 1024, 8, seed 0, refine 1, fix_scale 0, max_scale 0, min_gap 1e-6 */
int sg_slam_align_points(sg_slam* s, sg_map* map, const int32_t* corr /*[2M]: point a, point b*/,
                         const int32_t* group_offset /*[n+1]*/, int32_t n, const sg_align_options* options,
                         int32_t* solved /*[n]*/, sg_align_result* results /*[n], may be NULL*/,
                         int32_t* corr_inlier /*[M], may be NULL*/);

/* Applies the similarity Y = scale R(q) X + t to the listed frames and points of the map: the companion that makes a
 * loop correction one call after sg_slam_align_points.  Host only: no handle, no device.
 *   - each listed point: X <- [scale R X.xyz + t X.w, X.w], not renormalised;
 *   - each listed frame: t_f <- scale R t_f + t and q_f <- q_f (x) conj(q), renormalised with w >= 0.  Under the map's
 *     convention p = q_f (X - t_f) every camera-space point of a transformed frame on a transformed point is scaled by
 *     scale, so every pixel is unchanged.
 * q is normalised before use.  SG_EINVAL, with nothing written: a null map, q or t, or a null list with a positive
 * count; a negative count; q with | |q|^2 - 1 | > 1e-9 (zero and non-finite included); scale <= 0 or not finite; a
 * non-finite t; an index out of range or listed twice. */
int sg_map_apply_similarity(sg_map* map, double scale, const double* q /*[4]*/, const double* t /*[3]*/,
                            const int32_t* frames /*[nf]*/, int32_t nf, const int32_t* points /*[np]*/, int32_t np);

/* Match by projection: given a pose, which landmarks does this frame see?  sg_hamming_match compares every keypoint
 * with every descriptor of the map and ignores geometry; once sg_slam_localize_frames, sg_slam_optimize_pose_graph or
 * plain tracking has given a frame a pose, this call recovers the frame's other keypoints by a guided search: the
 * listed points are projected into each listed frame, and a keypoint's 256-bit descriptor (4 x u64, the convention
 * of sg_hamming_match) is compared only with the points that project inside a pixel window around it.  All frames of
 * a call run in three launches.  K = kp_offset[n]; the keypoints of the i-th listed frame f = frames[i] are
 * kp_offset[i] .. kp_offset[i + 1], pixels kp_xy[2 k], kp_xy[2 k + 1].
 *   1. Candidates of frame f: position j of points[] is a candidate when Project(q_f, t_f, k[frame_camera[f]],
 *      X[points[j]]) of csrc/project_math.h, in fp64, accepts it (not behind the camera: p.z >= 0.001 W), the projected
 *      u and v are finite, the projection lies in [0, width) x [0, height) when a bound is given (width = height = 0:
 *      no bound), and, with skip_observed, frame f has no observation of that point with obs_disabled == 0.  Point
 *      flags are not consulted (the convention of sg_slam_solve_points).  num_projected counts them.
 *   2. Window of keypoint k of frame f: the candidates with (u - x)^2 + (v - y)^2 <= radius_px^2, each product and
 *      the sum rounded once, in fp64.  A keypoint with a non-finite pixel has an empty window.
 *      num_candidates[k] is the window's size; best_point[k] the map index of the candidate with the smallest
 *      (popcount(kp XOR point), position j), or -1 for an empty window; best_dist[k] that popcount, or -1;
 *      second_dist[k] the second smallest distance of the window as a multiset (sg_hamming_match's rule: equal to
 *      best_dist on a tie), or -1 with fewer than two candidates.
 *   3. match[k], decided on the host from those arrays: keypoint k is accepted when best_point >= 0, best_dist <=
 *      max_dist and either second_dist < 0 or 100 best_dist <= ratio_percent second_dist (integers).  Within one listed
 *      frame, a point claimed by several accepted keypoints goes to the one with the smallest (best_dist, keypoint
 *      index); the other claimants get -1 (no fall-back to their second choice).  match[k] is a map point index or -1.
 *   4. results[i] (may be NULL): the frame's keypoints, its candidates, its keypoints with a non-empty window and its
 *      matches.  best_point, best_dist, second_dist and num_candidates may be NULL too.
 *   - A frame may be listed more than once, each time with its own keypoints.  A frame's results do not depend on its
 *     position in the call and are reproducible bit for bit.  With K == 0 or np == 0 nothing is launched and the
 *     outputs are the empty answers (-1, -1, -1, -1, 0; num_projected 0 too).  The map is never written; sg_slam_iterations, sg_slam_error
 *     and sg_slam_last_summary do not move.  No communicator is involved: rank-local on a sharded handle.
 *   - SG_EINVAL, all found on the host before the device is touched, with nothing written: a null s, map, options or
 *     match; n < 0 or np < 0; with n > 0 a null frames or kp_offset, a null kp_xy or kp_desc when K > 0, a null points
 *     or point_desc when np > 0; kp_offset[0] != 0 or a decreasing offset; a frame or point index out of range; a point
 *     listed twice; radius_px not above 0 or not finite; width or height negative, or only one of them zero; max_dist
 *     outside 0..256; ratio_percent outside 1..100; K > 2^20; n np > 2^22 (the index bits of the packed key, and a
 *     workspace near 200 MiB: split the frames over calls); a map whose poses, cameras or (np > 0) points cannot be
 *     read, a frame whose camera index is out of range; with skip_observed, a map whose observations cannot be read or
 *     whose observation indices are out of range.  n == 0 returns SG_OK before the handle or the device is touched.
 * Not in scope: scale or octave prediction and viewing-angle tests; a per-point radius; writing observations into the
 * map; a spatial grid. */
typedef struct sg_match_options {
  double radius_px;        /* > 0 and finite */
  int32_t width, height;   /* both > 0: a projection outside [0, width) x [0, height) is no candidate; both 0: no bound */
  int32_t max_dist;        /* 0..256 */
  int32_t ratio_percent;   /* 1..100 */
  int32_t skip_observed;   /* != 0: a point the frame already observes (obs_disabled == 0) is no candidate for it */
} sg_match_options;

typedef struct sg_match_result {
  int32_t num_keypoints, num_projected, num_with_candidates, num_matched;
} sg_match_result;

void sg_match_options_default(sg_match_options* o);   /* 12.0, 0, 0, 64, 80, 1 */
int sg_slam_match_by_projection(sg_slam* s, const sg_map* map, const int32_t* frames /*[n]*/, int32_t n,
                                const int32_t* kp_offset /*[n+1]*/, const double* kp_xy /*[2K]*/,
                                const uint64_t* kp_desc /*[4K]*/, const int32_t* points /*[np]*/, int32_t np,
                                const uint64_t* point_desc /*[4 np]*/, const sg_match_options* options,
                                int32_t* match /*[K]*/, int32_t* best_point /*[K], may be NULL*/,
                                int32_t* best_dist /*[K], may be NULL*/, int32_t* second_dist /*[K], may be NULL*/,
                                int32_t* num_candidates /*[K], may be NULL*/,
                                sg_match_result* results /*[n], may be NULL*/);

/* Match along epipolar lines: which still-unmatched keypoints of two posed frames are the same new landmark?
 * sg_slam_match_by_projection finds only points the map already has, and sg_hamming_match ignores geometry.  After a
 * keyframe is inserted, this call pairs the keypoints of frame a with those of frame b along the epipolar line their
 * stored poses give; sg_slam_triangulate_points then makes the landmarks.  All pairs of a call run in three launches.
 * Pair i = (pairs[2 i], pairs[2 i + 1]) brings its own keypoints: rows a_offset[i] .. a_offset[i + 1] of the a arrays
 * and b_offset[i] .. b_offset[i + 1] of the b arrays (KA = a_offset[n], KB = b_offset[n]), level-0 pixels, 256-bit
 * descriptors (4 x u64) and, optionally, the pyramid levels that sg_frontend_detect returns.  A frame listed in several
 * pairs is given its keypoints each time.
 *   1. Pair record, on the host in fp64: R_a and R_b from the stored quaternions by the matrix of ProjectJacobian
 *      (csrc/project_math.h; the quaternion is not normalised), R = R_b R_a^T, tr = R_b (t_a - t_b), E = [tr]x R
 *      (row-major), ifa = {1 / fx_a, 1 / fy_a} and ifb likewise: the map's convention p = R(q) (X - t W).  The pair is
 *      degenerate when an entry of E, R or tr is not finite or every entry of E is zero; it then has no candidates and
 *      results[i].degenerate = 1.
 *   2. Per keypoint: x = UndistortPixel(k_cam, pixel).  a side: l = E (x_a, 1), na = (l0 ifb0)^2 + (l1 ifb1)^2,
 *      g = R (x_a, 1).  b side: m = E^T (x_b, 1), nb = (m0 ifa0)^2 + (m1 ifa1)^2.
 *   3. b keypoint j is a candidate of a keypoint k when, in this order and with every comparison false on a NaN:
 *      the gate: r = x_b0 l0 + x_b1 l1 + l2, den = na + nb, den > 0 and r r <= tol_px^2 4^L den with L the larger of
 *      the two levels (0 without levels): RelSampson of csrc/relpose_math.h without the division; the depths: with
 *      f_b = (x_b, 1), RelDepths' det > 0 and the numerators of both depths > 0; and, with min_parallax > 0,
 *      RelParallax(g, x_b) >= min_parallax.
 *   4. num_candidates[k] is the number of candidates; best_kp[k] the candidate with the smallest (popcount(a XOR b),
 *      j), j being the b keypoint's index within the pair; best_dist[k] that popcount; second_dist[k] the second
 *      smallest distance as a multiset (equal to best_dist on a tie), -1 with fewer than two candidates.  The empty
 *      answers are -1, -1, -1, 0.
 *   5. match[k], decided on the host by sg_slam_match_by_projection's rule within each pair: accepted when best_kp >=
 *      0, best_dist <= max_dist and either second_dist < 0 or 100 best_dist <= ratio_percent second_dist; a b keypoint
 *      claimed by several accepted a keypoints goes to the smallest (best_dist, a index), the others get -1.  match[k]
 *      is a b index within the pair, or -1.
 *   - A pair's results do not depend on its position in the call and are reproducible bit for bit.  A pair without a
 *     or without b keypoints gives the empty answers; when every pair is empty or degenerate nothing is launched.  The
 *     map is never written; sg_slam_iterations, sg_slam_error and sg_slam_last_summary do not move.  No communicator is
 *     involved: rank-local on a sharded handle.  best_kp, best_dist, second_dist, num_candidates and results may be
 *     NULL.
 *   - SG_EINVAL, all found on the host before the device is touched, with nothing written: a null s, map, options or
 *     match; n < 0; with n > 0 a null pairs, a_offset or b_offset; a null xy or desc array whose count is above 0; only
 *     one of a_level and b_level given; a level outside 0..7; an offset array that does not start at 0 or decreases; a
 *     frame index out of range; a == b in a pair; a frame whose camera index is out of range; a map whose poses or
 *     cameras cannot be read; tol_px not above 0 or not finite; min_parallax negative or not finite; max_dist outside
 *     0..256; ratio_percent outside 1..100; KA or KB above 2^20; partial results above 128 MiB: the sum over the pairs
 *     of (a keypoints) x ceil(b keypoints / 512) above 2^23 (split the pairs over calls).  n == 0 returns SG_OK before
 *     the handle or the device is touched.
 * Not in scope: octave-consistency or orientation tests; an exclusion zone around the epipole (the parallax gate is the
 * guard); a symmetric cross-check; writing points or observations into the map; a spatial index. */
typedef struct sg_epipolar_options {
  double tol_px;          /* > 0 and finite: the gate, in ideal pixels (Sampson) */
  double min_parallax;    /* rad, >= 0 and finite; 0: no parallax test */
  int32_t max_dist;       /* 0..256 */
  int32_t ratio_percent;  /* 1..100 */
} sg_epipolar_options;

typedef struct sg_epipolar_result {
  int32_t num_a, num_b, num_with_candidates, num_matched, degenerate;
} sg_epipolar_result;

void sg_epipolar_options_default(sg_epipolar_options* o);   /* 2.0, 0.0, 64, 80 */
int sg_slam_match_epipolar(sg_slam* s, const sg_map* map, const int32_t* pairs /*[2n]: frame a, frame b*/, int32_t n,
                           const int32_t* a_offset /*[n+1]*/, const double* a_xy /*[2 KA]*/,
                           const uint64_t* a_desc /*[4 KA]*/, const int32_t* a_level /*[KA] or NULL*/,
                           const int32_t* b_offset /*[n+1]*/, const double* b_xy /*[2 KB]*/,
                           const uint64_t* b_desc /*[4 KB]*/, const int32_t* b_level /*[KB] or NULL*/,
                           const sg_epipolar_options* options, int32_t* match /*[KA]*/,
                           int32_t* best_kp /*[KA], may be NULL*/, int32_t* best_dist /*[KA], may be NULL*/,
                           int32_t* second_dist /*[KA], may be NULL*/, int32_t* num_candidates /*[KA], may be NULL*/,
                           sg_epipolar_result* results /*[n], may be NULL*/);

/* Pose-graph optimisation: spread a loop closure over the frames.  sg_slam_align_points gives the similarity that
 * joins two pieces of a map, and sg_map_apply_similarity moves one piece rigidly; but the drift of a long run is not a
 * rigid offset of one piece.  This call distributes it over the trajectory, scale included, so that the window solve
 * that follows starts inside its basin.  A call holds any number of graphs, one workgroup each, in one launch; graph g
 * has the nodes node_offset[g] .. node_offset[g + 1] and the edges edge_offset[g] .. edge_offset[g + 1].
 *   Nodes.  node_frame[i] is a map frame, node_fixed[i] != 0 holds it constant.  State: q (unit, the map's
 *     p = R(q)(X - t)), the centre t and the log-scale sigma, 0 for every node at entry; lambda = e^sigma is the local
 *     map scale at the frame: world-from-camera is p -> lambda R^T p + t.  A free node carries 7 unknowns: the rotation
 *     by ceres::QuaternionParameterization on Eigen memory (the one sg_slam_solve_frame_poses uses), t and sigma
 *     additive; with fix_scale 6: sigma stays 0 and the scale residual is dropped.
 *   Edges.  edge_ab[2 e], edge_ab[2 e + 1] are positions a != b in the graph's node list; edge_meas[8 e ..] is the
 *     measurement q^ (4), u^ (3), rho^; edge_weight[3 e ..] is w_rot, w_t, w_s (w_s is not read with fix_scale).  The
 *     residual, in fp64:
 *         q_e = conj(q^) (x) q_a (x) conj(q_b), sign-flipped to w >= 0;  omega = its rotation vector
 *         r[0:3] = w_rot omega;  r[3:6] = w_t (e^-sigma_a R_a (t_b - t_a) - u^);  r[6] = w_s (sigma_b - sigma_a - rho^)
 *     omega = 2 atan2(|v|, w) v / |v| with v the vector part of q_e; where |v|^2 < 1e-8 the factor comes from the series
 *     (2 / w)(1 - x^2 / 3 + x^4 / 5), x = |v| / w (csrc/posegraph_math.h, with the analytic 7 x 14 Jacobian).
 *     Loss: range > 0: CauchyLoss(range) on |r|^2 as everywhere else here (residual and Jacobian scaled by sqrt(rho'));
 *     range == 0: none.  Several edges between one pair are summed in listed order.  An edge between two fixed nodes
 *     goes into fixed_cost only.
 *   Solver.  The handle's sg_solver_options (sg_slam_set_options) on the Ceres 1.8 LM of sg_ba_solve: Jacobi scaling
 *     from iteration 0, the clamped LM diagonal, a sparse block Cholesky of the damped scaled system (a non-positive
 *     pivot makes an invalid step), the model cost change -sum_e (J_e d).(r_e + J_e d / 2) from the stored edge
 *     Jacobians, the same step decision.  The elimination order (greedy minimum degree, ties to the lower list
 *     position), the fill and every summation order are planned on the host (csrc/posegraph_plan.h); the whole LM loop
 *     of a graph runs in one workgroup of one launch, so a result is reproducible bit for bit and does not depend on
 *     the graph's position in the call.
 *   Status per graph, the first rule of sg_posegraph_status that applies.  Anything but SG_PG_OK leaves the graph's
 *     frames untouched.
 *   Write-back of an SG_PG_OK graph: q_f normalised with w >= 0 and t_f of its free nodes into the map; log_scale[i]
 *     (one per listed node of the call) receives sigma, 0 for fixed nodes and for graphs that are not OK.  With
 *     move_points != 0, on the host: every map point with an observation with obs_disabled == 0 in a node of an OK
 *     graph moves with its anchor, the node frame of its first such observation in map order:
 *         xyz <- lambda R_new^T R_old (xyz - W t_old) + W t_new,  W kept, not renormalised
 *     which leaves every pixel of the anchor frame on that point unchanged (a fixed anchor moves nothing).  Point flags
 *     and obs_disabled are neither read for gating nor written beyond that test.
 *   summaries (may be NULL) receives each graph's summary (SG_DID_NOT_RUN where the device did not run it).
 *     sg_slam_iterations grows by the num_iterations of the graphs that ran, and sg_slam_error / sg_slam_last_summary
 *     take the values of the last listed graph that ran (the convention of sg_slam_solve_frame_poses).
 *   - SG_EINVAL, all found on the host before the device is touched, with nothing written: a null s, map or options;
 *     n < 0; with n > 0 a null node_offset, edge_offset or status, a null node_frame or node_fixed when the call lists a
 *     node, a null edge_ab, edge_meas or edge_weight when it lists an edge; an offset array that does not start at 0 or
 *     decreases; a frame index out of range; a frame listed twice in the call; an edge index out of the graph's node
 *     list; a == b; q^ with | |q^|^2 - 1 | > 1e-9 (zero and non-finite included); a non-finite u^ or rho^; a weight that
 *     is not > 0 and finite (w_s only without fix_scale); range < 0, NaN or infinite; a map whose poses cannot be read;
 *     with move_points a map whose points or observations cannot be read or whose observation indices are out of
 *     range; more than 1024 nodes or 8192 edges in a graph; more than 65536 nodes, 32768 edges, 131072 blocks of the
 *     factors or 4194304 factor updates in a call (together these keep a call's device workspace under 256 MiB).
 *     n == 0 returns SG_OK before the handle or the device is touched.  A failing call writes nothing.
 * One graph occupies one workgroup, whatever its size: a 1000-node graph does not use more of the device than an
 * 8-node one.  No communicator is involved: rank-local on a sharded handle.
 * Not in scope: merging duplicated landmarks; information matrices beyond three weights; switchable constraints; any
 * multi-workgroup solve of one graph. */
enum sg_posegraph_status {
  SG_PG_OK = 0,            /* the solve finished with ok = 1 */
  SG_PG_DID_NOT_RUN = 1,   /* no free node, or no edge touches a free node (decided on the host) */
  SG_PG_NO_ANCHOR = 2,     /* a connected component that holds a free node holds no fixed node (decided on the host) */
  SG_PG_FAILED = 3         /* the solve ended with ok = 0 */
};

typedef struct sg_posegraph_options {
  double range;          /* CauchyLoss range on |r|^2; 0: no loss */
  int32_t fix_scale;     /* != 0: sigma = 0 everywhere, 6 unknowns per node */
  int32_t move_points;   /* != 0: move the map's points with their anchor frames (host) */
} sg_posegraph_options;

void sg_posegraph_options_default(sg_posegraph_options* o);   /* range 0, fix_scale 0, move_points 0 */
int sg_slam_optimize_pose_graph(sg_slam* s, sg_map* map, const int32_t* node_frame /*[N]*/,
                                const int32_t* node_fixed /*[N]*/, const int32_t* node_offset /*[n+1]*/,
                                const int32_t* edge_ab /*[2E]*/, const double* edge_meas /*[8E]*/,
                                const double* edge_weight /*[3E]*/, const int32_t* edge_offset /*[n+1]*/, int32_t n,
                                const sg_posegraph_options* options, int32_t* status /*[n]*/,
                                double* log_scale /*[N], may be NULL*/, sg_solver_summary* summaries /*[n], may be NULL*/);

/* The measurement of each listed frame pair (a, b) = pairs[2 i], pairs[2 i + 1] as the map stands: meas[8 i ..] =
 * q^ (4), u^ (3), rho^ of sg_slam_optimize_pose_graph.  Host only: no handle, no device; the map is not written.
 *   - sim == NULL: q^ = q_a (x) conj(q_b) (normalised, w >= 0), u^ = R_a (t_b - t_a), rho^ = 0: an odometry or
 *     covisibility edge, with zero residual at entry.
 *   - sim = scale, q[4], t[3] (8 doubles, exactly sg_align_result's Y = scale R(q) X + t from a's piece to b's): frame a
 *     is first moved as sg_map_apply_similarity would move it and takes the local scale s:
 *         t_a' = s R_S t_a + t_S,  q_a' = q_a (x) conj(q_S);
 *         q^ = q_a' (x) conj(q_b),  u^ = R_a' (t_b - t_a') / s,  rho^ = -ln s.
 *     This is the one place where an sg_slam_align_points result becomes a loop edge.
 * SG_EINVAL, with nothing written: a null map, or a null pairs or meas with n > 0; n < 0; a frame index out of range;
 * a == b; a map whose poses cannot be read; sim with the faults sg_map_apply_similarity refuses (scale <= 0 or not
 * finite, q not unit to 1e-9, a non-finite t). */
int sg_map_pose_edges(const sg_map* map, const int32_t* pairs /*[2n]*/, int32_t n, const double* sim /*[8] or NULL*/,
                      double* meas /*[8n]*/);

/* The pairs of listed frames that share at least min_shared slam-usable points through observations with
 * obs_disabled == 0 (the point filter of sg_slam_solve_frame_poses): candidates for covisibility edges.  Host only.
 * A pair is (i, j), i < j, positions in frames[]; pairs come in lexicographic order.  Two-call filling: *count is
 * always the full number, and at most cap pairs (2 cap ints) are written to pairs_out (may be NULL with cap == 0).
 * SG_EINVAL: a null map or count, a null frames with nf > 0, a null pairs_out with cap > 0; nf < 0, cap < 0,
 * min_shared < 1; a frame index out of range or listed twice; a map whose observations cannot be read or whose
 * observation indices are out of range. */
int sg_map_covisible_pairs(const sg_map* map, const int32_t* frames /*[nf]*/, int32_t nf, int32_t min_shared,
                           int32_t* pairs_out /*[2 cap]*/, int32_t cap, int32_t* count);

/* ------------------------------------------------------------------------------------------------
 * Front end: HessianTracker (hessian.h:9-270) and the forward/backward matching step of Matcher
 * (matcher.cpp:173-206 TrackFeature, 247-251 the 3 -> 6 level retry).  A tracker holds `max_images`
 * device pyramids ("views", matcher.cpp:36-40); images are 8-bit, 3 channels, cv::Mat (BGR) memory order.
 */
typedef struct sg_tracker sg_tracker;

typedef struct sg_tracker_options {
  int32_t window;          /* patch size W: kWindowSize = 13 (matcher.cpp:27); 1..16 */
  int32_t depth;           /* pyramid levels per image: MakePyramid(img, 6) (matcher.cpp:221); 1..8 */
  int32_t max_iterations;  /* Track() Newton iterations: 10 (matcher.cpp:176) */
  float threshold;         /* Track() convergence threshold: 0.001 (matcher.cpp:176) */
  float fb_max;            /* forward/backward disagreement limit: 0.3 px (matcher.cpp:200) */
  int32_t retry_levels;    /* levels of the retry after a failed attempt: 6 (matcher.cpp:248); 0 = none */
  int32_t max_images;      /* pyramid slots held on the device */
  int32_t mode;            /* FeatureTracker implementation: SG_TRACKER_HESSIAN (the one Matcher uses,
                              matcher.cpp:20), SG_TRACKER_KLT (klt.h), SG_TRACKER_BRUTE (brute.h) */
  int32_t reserved[4];
} sg_tracker_options;

enum sg_tracker_mode { SG_TRACKER_HESSIAN = 0, SG_TRACKER_KLT = 1, SG_TRACKER_BRUTE = 2 };

void sg_tracker_options_default(sg_tracker_options* o);
int sg_tracker_create(sg_tracker** out, const sg_tracker_options* o, const sg_device_options* dev);
void sg_tracker_destroy(sg_tracker* t);

/* MakePyramid (hessian.h:95-126) of one image into pyramid slot `slot`.  `stride` is bytes per row (cv::Mat's
 * step), stride >= 3 * width (SG_EINVAL otherwise).  Bytes past 3 * width in a row are never read: the image may be
 * a view into a wider one whose last row ends at the end of its allocation (stride * (height - 1) + 3 * width
 * readable bytes suffice).  sg_frontend_track's image follows the same rule. */
int sg_tracker_set_image(sg_tracker* t, int32_t slot, const uint8_t* bgr, int32_t width, int32_t height,
                         int32_t stride);
/* Download pyramid level `level` of slot `slot` (width*height floats). */
int sg_tracker_get_level(sg_tracker* t, int32_t slot, int32_t level, float* out, int32_t* width,
                         int32_t* height);
/* GetPatch (hessian.h:54-93) at n points of one level: out[n][W*W], mean[n], sumsq[n]. */
int sg_tracker_get_patches(sg_tracker* t, int32_t slot, int32_t level, int32_t n, const float* xy, float* out,
                           float* mean, float* sumsq);
/* Forward/backward tracking of n features from slot `from` to slot `to` (synchronous).  levels[i] is 3 or 6
 * (matcher.cpp:234-236); to_xy: in = starting guess, out = the matcher's to_pt; accepted[i] = 1 if the
 * feature matched; iterations (may be NULL) = Newton iterations spent per feature. */
int sg_tracker_track(sg_tracker* t, int32_t from, int32_t to, int32_t n, const float* from_xy, float* to_xy,
                     const int32_t* levels, int32_t* accepted, int32_t* iterations);
/* Device-resident variant for throughput runs: load features once, run `repeats` asynchronous tracking
 * passes (each restarts from the loaded starting guesses), then fetch the last pass's results. */
/* One-directional TrackFeature of the tracker's mode for n features (hessian.h:243-264, klt.h:403-424,
 * brute.h:129-164): templates GetPatches(from slot, from_xy) (levels[i] of them in HESSIAN mode, NULL = all;
 * every level in the other modes), then coarse-to-fine tracking in the `to` slot starting from to_xy, with
 * threshold / max_iterations from the options.  to_xy is updated only where status is 0 (OK); 2 =
 * OUT_OF_BOUNDS.  iterations (optional): Newton iterations run (0 in BRUTE mode). */
int sg_tracker_track_feature(sg_tracker* t, int32_t from, int32_t to, int32_t n, const float* from_xy, float* to_xy,
                             const int32_t* levels, int32_t* status, int32_t* iterations);
int sg_tracker_load_features(sg_tracker* t, int32_t n, const float* from_xy, const float* to_xy,
                             const int32_t* levels);
int sg_tracker_run(sg_tracker* t, int32_t from, int32_t to, int32_t repeats);
int sg_tracker_results(sg_tracker* t, float* to_xy, int32_t* accepted, int32_t* iterations);
/* New-keyframe corner seeding of Matcher::Track (matcher.cpp:123-169, 214, 380-383) on the image of `slot`:
 * grey = cvtColor(BGR, CV_RGB2GRAY); goodFeaturesToTrack(grey, max_corners = 120, quality = 0.01,
 * min_distance = 20) (Shi-Tomasi, blockSize 3, strongest first, ties in row-major order); then
 * AddNewFeatures' 30 x 30 grid: a corner is added unless its cell is within one cell of a match.
 * corners_xy / added_xy hold up to max_corners points each (x, y). */
int sg_tracker_seed_features(sg_tracker* t, int32_t slot, const float* match_xy, int32_t num_matches,
                             int32_t max_corners, double quality, double min_distance, float* corners_xy,
                             int32_t* num_corners, float* added_xy, int32_t* num_added);
/* Kernel timing (HIP events on the tracker's stream) of the last sg_tracker_run: total ms of the
 * tracking kernels and of the pyramid kernels of the last sg_tracker_set_image. */
int sg_tracker_kernel_ms(sg_tracker* t, double* track_ms, double* pyramid_ms);

/* Describe keypoints: oriented 256-bit descriptors (a steered BRIEF of this project's own pattern,
 * csrc/brief_pattern.h) read from the blurred float pyramid of slot `slot`, as the 4 x uint64 rows that
 * sg_hamming_match and sg_slam_match_by_projection consume.  One device launch per call, keypoints on any levels.
 * For keypoint i on level l = levels[i] (NULL = all 0) of size w_l x h_l:
 *   centre  px = x 2^-l, py = y 2^-l in fp32 (exact); cx = (int)floorf(px + 0.5f), cy likewise.  SG_DESC_BORDER when
 *           x or y is not finite, or cx < 15, cx > w_l - 16, cy < 15 or cy > h_l - 16 (a level narrower or lower
 *           than 31 refuses every keypoint); a refused keypoint gets four zero words and angle_bin -1.
 *   moments m10 = sum u I(cx + u, cy + v), m01 = sum v I(cx + u, cy + v) over the 709 pixels u^2 + v^2 <= 15^2, in
 *           fp64 (every product is exact), in a fixed order without atomics: the same bits on every run and
 *           wherever the keypoint stands in the call.
 *   bin     angle_bin = 0 when m10 == 0 && m01 == 0, else the k in 0..31 whose direction 2 pi k / 32 is nearest
 *           to atan2(m01, m10), image y pointing down (csrc/describe_math.h: the argmax over k of
 *           fma(m10, cos_k, m01 * sin_k) on a constant table, ties to the lower k).
 *   bits    bit j & 63 of word j >> 6 is I(cx + ax, cy + ay) < I(cx + bx, cy + by) on the float pixels for row
 *           (ax, ay, bx, by) = pattern[k][j]; false on a tie.
 * SG_EINVAL, found on the host before the device is touched and with nothing written: a null handle, n < 0,
 * n > 2^20, null xy or desc with n > 0, a slot out of range or never set, a level outside 0..depth-1.  n == 0 returns
 * SG_OK and launches nothing. */
enum sg_describe_status { SG_DESC_OK = 0, SG_DESC_BORDER = 1 };
int sg_tracker_describe(sg_tracker* t, int32_t slot, int32_t n, const float* xy /*[2n], level-0 pixels*/,
                        const int32_t* levels /*[n], NULL = all 0*/, uint64_t* desc /*[4n]*/,
                        int32_t* angle_bin /*[n], may be NULL*/, int32_t* status /*[n], may be NULL*/);
/* HIP events around the last describe launch of this tracker. */
int sg_tracker_describe_ms(sg_tracker* t, double* kernel_ms);

/* Detect keypoints: FAST-9 corners on the blurred float pyramid of slot `slot`, spread over the image by 32 x 32
 * cells, on any range of levels in one device launch.  The output goes straight into sg_tracker_describe.  The rules
 * apply to each selected level l, whose image I has size w x h.  Every decision is an fp32 comparison, a min or a
 * max; there is no sum and no product, so the answer has no rounding freedom (csrc/detect_math.h holds the shared
 * arithmetic).
 *   ring       the 16 offsets (dx, dy) of the radius-3 Bresenham circle, clockwise from the top:
 *              (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2)
 *              (-1,-3).
 *   score      d_i = I(ring_i) - I(p), one fp32 subtraction;
 *              s(p) = max( max_k min_{j<9} d_{(k+j)&15} , max_k min_{j<9} (-d_{(k+j)&15}) ): the largest threshold at
 *              which p is still a FAST-9 corner, bright or dark.  Defined wherever the ring fits, which with
 *              border >= 4 covers every neighbour of an admissible pixel.
 *   candidate  p = (x, y) is admissible when border <= x <= w-1-border and border <= y <= h-1-border (a level too
 *              small for that yields nothing).  An admissible p is a candidate when s(p) > t_lo and it survives the
 *              3 x 3 non-maximum suppression: s(p) > s of the four neighbours earlier in row-major order (the three
 *              above and the left one) and s(p) >= s of the four later ones.  Neighbours outside the admissible
 *              rectangle take part with their real score.  No two 8-adjacent pixels both survive, so a cell holds at
 *              most 256 candidates.
 *   cells      32 x 32 level pixels, anchored at pixel (0, 0) of the level; the last column and row may be partial.
 *              If a cell has a candidate with s > t_hi, only those candidates are eligible; otherwise all its
 *              candidates are, and a cell that has candidates but none above t_hi counts in low_cells (a cell
 *              without candidates is on neither branch).  The cell keeps its per_cell best eligible candidates by
 *              (s descending, pixel index y w + x ascending).
 *   output     xy = (x 2^l, y 2^l), exact in fp32, so that sg_tracker_describe recovers exactly (x, y) on level l;
 *              levels = l; score = s.  Order: level ascending, then cell row-major, then rank within the cell.
 *   cap        with max_keypoints > 0 and more keypoints than that, the max_keypoints best of the call by
 *              (s descending, level ascending, pixel index ascending) stay; the output order is unchanged.
 *   filling    *count is always the full number of keypoints (after the cap of max_keypoints); at most `cap` of
 *              them, the first in output order, are written, and array elements past those are left as they were.
 *              cap == 0 with null arrays is allowed.  cap >= (sum of the selected levels' cells) x per_cell always
 *              holds everything.
 *   per_level  [depth] records (may be NULL): every level's width and height; for the selected levels also the
 *              number of cells, the candidates before selection, low_cells, and the keypoints after the cap; the
 *              other fields of levels that were not selected are 0.
 * The same bits come out on every run and wherever the image sits in a slot: no atomics, no order-dependent step.
 * SG_EINVAL, found on the host before the device is touched and with nothing written: a null handle, options or
 * count; cap < 0; null xy or levels with cap > 0; a slot out of range or never set; first_level outside
 * 0..depth-1; num_levels < 0 or first_level + num_levels > depth; a threshold that is not finite or is negative, or
 * min_threshold > threshold; border outside 4..64; per_cell outside 1..16; max_keypoints < 0.
 * Not built: sub-pixel refinement, a Harris ranking, a quadtree distribution; the keypoints come back to the host. */
typedef struct sg_detect_options {
  float threshold;        /* t_hi, intensity units of the pyramid (grey / 255); default 20/255 */
  float min_threshold;    /* t_lo, 0 <= t_lo <= t_hi, finite; default 7/255 */
  int32_t first_level;    /* default 0 */
  int32_t num_levels;     /* 0 = every level from first_level to depth - 1 */
  int32_t border;         /* 4..64 level pixels; default 15 (sg_tracker_describe's) */
  int32_t per_cell;       /* 1..16; default 4 */
  int32_t max_keypoints;  /* 0 = no cap */
} sg_detect_options;
typedef struct sg_detect_level {
  int32_t width, height, cells, candidates, low_cells, keypoints;
} sg_detect_level;
void sg_detect_options_default(sg_detect_options* o);
int sg_tracker_detect(sg_tracker* t, int32_t slot, const sg_detect_options* o, int32_t cap,
                      float* xy /*[2 cap], level-0 pixels*/, int32_t* levels /*[cap]*/,
                      float* score /*[cap], may be NULL*/, int32_t* count,
                      sg_detect_level* per_level /*[depth], may be NULL*/);
/* HIP events around the last detect launch of this tracker. */
int sg_tracker_detect_ms(sg_tracker* t, double* kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * All-pairs 256-bit descriptor matching (the matcher's brute-force descriptor distance; BASELINE config 4).
 * Descriptors are 4 x uint64 per row.  Per query row: best_idx = argmin over train rows of
 * popcount(q XOR t) with ties to the lowest index, best_dist, and second_dist = the second-smallest
 * distance (equal to best_dist on a tie); -1 where the train set is too small.
 */
typedef struct sg_matcher sg_matcher;
int sg_matcher_create(sg_matcher** out, const sg_device_options* dev);
void sg_matcher_destroy(sg_matcher* m);
int sg_hamming_match(sg_matcher* m, const uint64_t* query, int32_t nq, const uint64_t* train, int32_t nt,
                     int32_t* best_idx, int32_t* best_dist, int32_t* second_dist);
/* Device-resident throughput path: load once, run `repeats` asynchronous passes, fetch results and the
 * average kernel time per pass (HIP events). */
int sg_hamming_load(sg_matcher* m, const uint64_t* query, int32_t nq, const uint64_t* train, int32_t nt);
int sg_hamming_run(sg_matcher* m, int32_t repeats);
int sg_hamming_results(sg_matcher* m, int32_t* best_idx, int32_t* best_dist, int32_t* second_dist,
                       double* kernel_ms);

/* Keyframe retrieval: which keyframe does this frame look like?  A device-resident database of keyframe descriptor
 * sets on the sg_matcher handle, and a query that matches one frame's descriptors against every stored set in one
 * call: three launches whatever the number of sets.  The query scores every set by its one-to-one matches, ranks the
 * sets, and returns the keypoint-to-keypoint matches of the best k.  Brute force and exact: integers only, the same
 * bits on every run.
 *
 * sg_matcher_db_add appends one keyframe's n descriptors (4 x uint64 per row) as set S; sets are numbered 0, 1, 2, ...
 * in order of addition and the number is returned in *set_id (may be NULL).  n == 0 makes an empty set.  The
 * descriptors are uploaded once and stay on the device; the device buffer grows geometrically, the old contents
 * moved by a device-to-device copy on the matcher's stream.  SG_EINVAL, with nothing changed: a null m; n < 0; a null
 * desc with n > 0; n > 65536; a 4097th set; more than 2^22 descriptors in all (128 MiB).
 * sg_matcher_db_clear forgets every set (numbering restarts at 0; the device buffer is kept).
 * sg_matcher_db_count gives the number of sets and of descriptors (either pointer may be NULL).
 *
 * sg_matcher_db_query, with S sets of n_s descriptors and nq query rows:
 *   1. For every set s with skip == NULL or skip[s] == 0 and every query row i: (best_idx, best_dist, second_dist)
 *      within set s alone by sg_hamming_match's rule: best_idx = argmin of popcount(q XOR t), ties to the lowest
 *      index within the set; second_dist = the second smallest distance of the multiset, -1 when n_s < 2.  An empty
 *      set gives no result.
 *   2. Query i is a candidate for set s when n_s >= 1, best_dist <= max_dist and either second_dist < 0 or
 *      100 best_dist <= ratio_percent second_dist (sg_slam_match_by_projection's acceptance rule, in integers).
 *   3. One-to-one within a set: a descriptor that is best_idx of several candidates goes to the candidate with the
 *      smallest (best_dist, i); the other claimants are unmatched in that set (no fall-back to a second choice).
 *   4. score[s] = the number of matched queries of set s (= the number of claimed descriptors); 0 for an empty set,
 *      -1 for a skipped one.
 *   5. Ranking, on the host: the sets with score >= min_score that are not skipped, by (score descending, set index
 *      ascending); top_set[r], top_score[r] hold the r-th of them for r < k, the remaining entries -1, -1.
 *   6. For each rank r with top_set[r] >= 0: match[r nq + i] = the index within the set of the descriptor matched to
 *      query i, or -1; match_dist[r nq + i] its distance, or -1.  Rows of unfilled ranks are -1.  Only the rows of
 *      the ranked sets are copied back from the device.  match and match_dist may be NULL.
 *   - A set's score and match row depend on the query, the options and that set's descriptors only: not on its
 *     position in the database, on the other sets or on skip; they are reproducible bit for bit.
 *   - With nq == 0 or S == 0 nothing is launched and the outputs are the empty answers: score 0 (-1 for a skipped
 *     set), ranked by rule 5 like any other scores (so nothing ranks unless min_score == 0).
 *   - sg_hamming_load / run / results / match on the same handle are independent of the database, and the reverse.
 *   - SG_EINVAL, all found on the host before anything is launched, with nothing written: a null m or options; a
 *     null score with S > 0; nq < 0; a null query with nq > 0; k < 0; a null top_set or top_score with k > 0;
 *     max_dist outside 0..256, ratio_percent outside 1..100, min_score < 0; nq > 2^20; S nq > 2^23.
 *   - Device workspace of a query, besides the database (32 bytes per descriptor) and the query: 8 S nq bytes of
 *     per-(set, query) cells (<= 64 MiB), 4 bytes per database descriptor of claims (<= 16 MiB), 4 S bytes of scores,
 *     and 8 bytes per (slice, query) of partials, <= 128 MiB: a set is cut into slices of 1024 descriptors, and the
 *     slice length doubles until slices x nq <= 2^24.  Buffers are kept between calls and grow geometrically.
 * sg_matcher_db_query_ms: HIP-event time of the last query's launches (0 when it launched nothing); SG_EINVAL before
 * the first query.
 * Not in scope: removing a single set (use skip); a vocabulary or an inverted index; geometric verification (that is
 * sg_slam_relative_poses / sg_slam_localize_frames); storing descriptors in sg_map; a symmetric cross-check. */
int sg_matcher_db_add(sg_matcher* m, const uint64_t* desc /*[4 n]*/, int32_t n, int32_t* set_id);
int sg_matcher_db_clear(sg_matcher* m);
int sg_matcher_db_count(const sg_matcher* m, int32_t* num_sets, int64_t* num_descriptors);
typedef struct sg_retrieve_options {
  int32_t max_dist;        /* 0..256 */
  int32_t ratio_percent;   /* 1..100 */
  int32_t min_score;       /* >= 0: a set ranks only with score >= min_score */
} sg_retrieve_options;
void sg_retrieve_options_default(sg_retrieve_options* o);   /* 64, 80, 1 */
int sg_matcher_db_query(sg_matcher* m, const uint64_t* query /*[4 nq]*/, int32_t nq,
                        const sg_retrieve_options* options, const uint8_t* skip /*[S] or NULL*/,
                        int32_t* score /*[S]*/, int32_t k, int32_t* top_set /*[k]*/, int32_t* top_score /*[k]*/,
                        int32_t* match /*[k nq], may be NULL*/, int32_t* match_dist /*[k nq], may be NULL*/);
int sg_matcher_db_query_ms(sg_matcher* m, double* kernel_ms);
int sg_slam_set_options(sg_slam* s, const sg_solver_options* o);

/* LocalMap maintenance on the device, run on the residuals sg_slam_reproject_map wrote (main.cpp:584-599).
 * A point's observation order (TrackedPoint::observations()) is ascending frame index, ties by map index
 * (Frame::Commit, localmap.cpp:85-89). */
/* LocalMap::Clean(error_threshold) (localmap.cpp:283-398): fixes X[4p+3], writes point_flags,
 * point_uncertainty and obs_disabled; *result = the reference's bool (0 when observations were disabled). */
int sg_map_clean(sg_slam* s, sg_map* map, double error_threshold, int32_t* result);
/* LocalMap::ApplyEpipolarConstraint() (localmap.cpp:232-276): writes point_flags and obs_disabled;
 * *num_violations = points whose |h2^T E h1| exceeded 0.15. */
int sg_map_apply_epipolar(sg_slam* s, sg_map* map, int32_t* num_violations);
/* LocalMap::Normalize (localmap.cpp:114-155): translate frame 0 to the origin, then rotate frame 0 to the
 * identity (frames' rotations and translations, points' homogeneous locations; a map with < 2 frames is left
 * alone).  main.cpp:602-605 checks that ReprojectMap is unchanged by it (CHECK_NEAR 0.1). */
int sg_map_normalize(sg_slam* s, sg_map* map);

/* ------------------------------------------------------------------------------------------------
 * Matcher::Track (matcher.h:20-26, matcher.cpp:301-405): the per-frame front end with its bookkeeping —
 * live features (ordered by TrackedPoint id), up to four keyframe views whose pyramids stay resident on the
 * device, FindMatches (matcher.cpp:210-271) batched over features on the device, the keyframe decision
 * (< 40 matches), corner seeding of new points (AddNewFeatures + Unproject at 2000) and view expiry.
 * The LocalMap stays the caller's: the library reads and grows it through these callbacks, which stand in
 * for the reference's direct member access (each cites what it replaces).  Callbacks return 0 on success;
 * a non-zero return aborts the call with SG_EINVAL.
 */
typedef struct sg_map_callbacks {
  void* user;
  /* Frame::rotation().coeffs() [x,y,z,w], translation(), camera()->k (localmap.h:129-132,159-160,30) */
  int32_t (*frame_pose)(void* user, int32_t frame, double* q4, double* t3, double* k7);
  /* TrackedPoint::location(), uncertainty(), feature_usable() (localmap.h:194-195,251,249) */
  int32_t (*point_state)(void* user, int32_t point, double* X4, double* uncertainty, int32_t* feature_usable);
  /* LocalMap::AddPoint(id, location) (localmap.cpp:103-109): NO_OBSERVATIONS | NO_BASELINE flags,
   * uncertainty 1e8.  Writes the new point's handle to *point. */
  int32_t (*add_point)(void* user, int32_t id, const double* X4, int32_t* point);
  /* Frame::AddObservation(pt, point) (localmap.h:138-143) */
  int32_t (*add_observation)(void* user, int32_t frame, double x, double y, int32_t point);
  /* frame->is_keyframe_ = true (matcher.cpp:357) */
  int32_t (*set_keyframe)(void* user, int32_t frame);
  /* Matcher::Track's update_frames argument (may be NULL): *updated = its bool result */
  int32_t (*update_frames)(void* user, int32_t* updated);
} sg_map_callbacks;

typedef struct sg_frontend_stats {
  int32_t matches_first;   /* "Started with %d" (matcher.cpp:341) */
  int32_t matches;         /* "grew to %d" */
  int32_t keyframe;        /* 1 when the frame became a keyframe */
  int32_t corners;         /* goodFeaturesToTrack corners on a keyframe */
  int32_t added;           /* new features / points ("Added %d new features") */
  int32_t features;        /* live features after the call */
  int32_t views;           /* keyframe views after the call */
  int32_t track_batches;   /* device FindMatches launches (one per pass; a second after update_frames) */
} sg_frontend_stats;

typedef struct sg_frontend sg_frontend;
/* o: tracker options (window 13, depth 6 for the reference's Matcher; NULL = defaults). */
int sg_frontend_create(sg_frontend** out, const sg_tracker_options* o, const sg_device_options* dev);
void sg_frontend_destroy(sg_frontend* f);
/* Matcher::Track(img, frame, camera, map, update_frames): *result = the reference's bool (always 1). */
int sg_frontend_track(sg_frontend* f, const uint8_t* bgr, int32_t width, int32_t height, int32_t stride,
                      int32_t frame, int32_t camera, const sg_map_callbacks* cb, int32_t* result,
                      sg_frontend_stats* stats);
/* Live features: point handles and TrackedPoint ids in set order (ids ascending); n in/out = capacity/count. */
int sg_frontend_features(sg_frontend* f, int32_t* points, int32_t* ids, int32_t* n);
/* sg_tracker_describe on the pyramid of the keyframe view the front end holds for `frame` (a frame that became a
 * keyframe and has not expired: at most the last four); SG_EINVAL when no view of that frame is held.  It reads
 * the view only: sg_frontend_track behaves as if the call had not been made. */
int sg_frontend_describe(sg_frontend* f, int32_t frame, int32_t n, const float* xy, const int32_t* levels,
                         uint64_t* desc, int32_t* angle_bin, int32_t* status);
/* sg_tracker_detect on the pyramid of the keyframe view held for `frame`, under sg_frontend_describe's rule:
 * SG_EINVAL when no view of that frame is held; it reads the view only. */
int sg_frontend_detect(sg_frontend* f, int32_t frame, const sg_detect_options* o, int32_t cap, float* xy,
                       int32_t* levels, float* score, int32_t* count, sg_detect_level* per_level);

#ifdef __cplusplus
}
#endif
#endif /* SLAMGPU_H_ */
