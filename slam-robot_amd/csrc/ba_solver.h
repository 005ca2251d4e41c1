// ba_solver.h — host driver of the MI355X bundle-adjustment solver (one per sg_ba handle).
#ifndef SG_BA_SOLVER_H_
#define SG_BA_SOLVER_H_

#include <hip/hip_runtime.h>

#include <chrono>
#include <memory>
#include <string>
#include <vector>

#include "ba_chain.h"
#include "ba_kernels.h"
#include "ba_plan.h"
#include "common.h"
#include "dbuf.h"
#include "hostio.h"
#include "hostmirror.h"

namespace sg {

void ValidateProblem(const sg_problem* p);

class Comm;  // RCCL communicator (comm.cpp)

class BaSolver {
 public:
  explicit BaSolver(const sg_device_options& dev);
  ~BaSolver();

  void Load(const sg_problem& p);
  // Pre-size every buffer that scales with the problem for up to F frames, P points and M observations (a
  // map's high-water mark), so that a later Load does not reallocate on its critical path.  Reallocating
  // drops the loaded structure (the next Load is a full one).
  void Reserve(int F, int P, int M);
  void Begin(const sg_solver_options& o);
  void Iterate(int n);
  void Sweep(int n);
  void Sync();
  void Summary(sg_solver_summary* s);
  void Download(sg_problem* p);
  void Solve(const sg_solver_options& o, sg_problem* p, sg_solver_summary* s);
  void Evaluate(double* residuals, double* cost, int32_t* nfail);
  void SetTiming(bool on);
  int KernelTimes(char* names, int names_len, double* ms, int32_t* counts, int max);
  int KernelWork(double* bytes, double* flops, int max);
  void CommInit(const void* id128, int nranks, int rank);
  void CommInitLocal(std::shared_ptr<struct LocalGroup> g, int rank);   // in-process test group (comm.h)
  void CommInitHost(int nranks, int rank, int (*fn)(double*, long long, int, void*), void* user);   // comm.h
  static void UniqueId(void* id128);

  void Info(sg_ba_info* out) const;

  // ReprojectMap (slam.cpp:523-548) over a whole map; used by the Slam facade.
  double ReprojectMap(sg_map* m);

  hipStream_t stream() const { return stream_; }
  int nranks() const;

 private:
  sg_device_options dev_;
  hipStream_t stream_ = nullptr;
  HostMirror mb_;   // mapped mailbox: [0, 1 KB) the LM state read back, then the solution download
  void ReadState(LmState* h);   // LmState via mb_ (a kernel writes it: no copy engine), stream synchronised
  void WaitStream(hipStream_t s);   // spin-wait for the stream's work (see ba_solver.hip)
  hipEvent_t ev_wait_ = nullptr;
  void EnqueueIterations(int n);
  hipEvent_t dev_marks_[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // SG_HOST_TIMING: device times in Load
  hipEvent_t ev_idle_ = nullptr;                                            //   the stream last seen idle (MarkIdle)
  hipEvent_t ev_idle_prev_ = nullptr;                                       //   the previous call's, at a load
  std::chrono::steady_clock::time_point idle_host_;
  bool idle_valid_ = false;
  void MarkIdle(hipStream_t s);
  void DevMark(hipStream_t s, int i);
  std::string LoadDeviceTimes(std::chrono::steady_clock::time_point load_t0, bool idle_valid_prev,
                              double idle_gap_host);
  bool need_seq_ = true;   // the next iteration is the first of a solve (it computes the camera scale)
  std::unique_ptr<Comm> comm_;
  bool loaded_ = false;
  bool began_ = false;
  // what the last full load planned (ba_plan.h): the Cholesky kernel choice and the counts of the work lists
  // and of the envelope
  CholPlan chol_;
  WorkCounts wk_;
  EnvCounts env_;
  size_t border_lds_max_ = 0;  // k_chol_border's dynamic LDS limit
  DBuf<double> Wg_;            // k_chol_tiles' back-substitution tiles W_KJ = U_KK^-1 U_KJ (+ the bottom half's)
  DBuf<int32_t> tflag_;        // dissected band hand-off counters {bottom done, top done}
  RunKnobs knobs_;   // the switches read at construction (ba_chain.h)
  bool chol_stile_last_ = false;   // the last LM iteration enqueued loaded k_S_reduce's tile-major copy of S
                                   // (sg_ba_info.cholesky_stile)
  size_t jslot_ = 0, cslot_ = 0;   // doubles per slot of J and cam_slab
  size_t ntail_ = 0;   // doubles of the merged exchange's tail
  bool pending_decision_ = false;   // speculative chain: the last enqueued step awaits its decision
  int32_t nallreduce_ = 0;   // landmark-shard all-reduces issued (sg_ba_info.num_allreduces)
  bool stamp_on_ = false;
  int wt_stores_ = 0;                   // Dev::wt of the last full load (SG_WT_STORES)
  int ncu_ = 256;                       // compute units (Schur segment count), queried once
  size_t tile_lds_set_ = 0;             // dynamic LDS last granted to k_chol_tiles
  size_t gchol_lds_max_ = 0;            // dynamic LDS granted to k_cholesky_global
  std::unique_ptr<class Stager> stager_;   // batched structure uploads (stager.h)
  DBuf<unsigned long long> stamps_;

 public:
  // diagnostic: per-phase cycle counters of the stamped kernels (SG_STAMP=1)
  std::vector<unsigned long long> Stamps();

 private:
  // host copies of the structure
  int F_ = 0, P_ = 0, M_ = 0, NB_ = 0, n_ = 0, D_ = 0, ncam_ = 0;
  std::vector<int32_t> point_perm_;   // device order -> problem point
  std::vector<int32_t> obs_perm_;     // device order -> problem observation
  // Incremental problem update (replacing the per-call rebuild of slam.cpp:257-414):
  // the structure of the last Load.  A Load with the same structure (frames, cameras, freedom flags,
  // observation -> frame / point incidence, FrameDistance pairs) keeps the point order, the CSR, the sweep
  // chunks, Schur segments, pair and reduction lists and the Cholesky envelope, and uploads the values only.
  struct StructKey {
    int32_t ncam = -1, cams_free = 0, F = -1, P = -1, M = -1, D = -1;
    std::vector<int32_t> frame_camera, obs_frame, obs_point, dist_frame, dist_prev;
    std::vector<uint8_t> rot_free, trans_free, point_free;
  } skey_;
  int32_t full_loads_ = 0, value_loads_ = 0;
  bool SameStructure(const sg_problem& p) const;
  void SaveStructure(const sg_problem& p);
  void LoadValues(const sg_problem& p);
  void ResetState(hipStream_t s);

 public:
  // loads that rebuilt the structure / loads that re-uploaded values only
  void LoadCounts(int32_t* full, int32_t* values) const {
    *full = full_loads_;
    *values = value_loads_;
  }

 private:
  // device buffers
  DBuf<LmState> st_;
  DBuf<double> k_, q_, t_, X_, obs_pt_, J_, V_, g_, scale_p_, diag_p_, Vinv_, tp_, scale_c_, diag_c_, camdiag_,
      camg_, cam_slab_, S_slab_, chunk_scal_, cam_wide_, S_wide_, xchg_cam_, S_, rhs_, xchg_upd_,
      xchg_chol_, work_, fd_r_, fd_J_, fd_D_, fd_X_, red_, zpre_;
  DBuf<int32_t> frame_cam_, frame_block_, poff_, obs_frame_, fd_a_, fd_b_, fd_boff_, fd_bidx_, cam_loff_,
      cam_lidx_, s_loff_, s_lidx_, r_loff_, r_lidx_, mobs_frame_, mobs_point_, mframe_cam_;
  DBuf<uint8_t> rot_free_, trans_free_, pfree_, obs_fixed_;
  DBuf<int32_t> work_i_;   // Cholesky panel envelopes (panel_jmax)
  DBuf<int32_t> fd_pair_;
  DBuf<int32_t> pu_units_;   // k_point_update work units
  DBuf<int32_t> pack_off_;   // per panel offset of its band rows in the packed all-reduce buffer
  DBuf<double> Spk_;         // packed band of S + rhs (landmark shards)
  DBuf<int32_t> obs_pnt_, pairs_;   // Schur work lists
  DBuf<int32_t> obs_meta_;         // packed per-observation facts (kMeta*)
  DBuf<double> Jk_, KU_, kst_;     // free intrinsics (nk_ > 0)
  DBuf<double> Yk_, kpart_;        //   W_kp V~p^-1 per point and camera; per-block camera sums
  DBuf<int32_t> intr_boff_, intr_bidx_;   //   per-block observation lists
  int nk_ = 0;                     // 7 * cameras when the intrinsics are free
  double stab_b_ = 25.0;
  DBuf<SchurSeg> segs_;
  DBuf<LinChunk> lchunks_d_;
  DBuf<LinRound> lrounds_d_;
  DBuf<double> lin_scal_;
  void LaunchLinearize(const Dev& d);
  void LaunchUpdateLin(const Dev& d);
  DBuf<double> seg_fail_;
  DBuf<SchurBatch> sbatch_;
  DBuf<WideSeg> wsegs_;
  DBuf<int32_t> pinfo_, pmx_, cells_, cell_obs_, stile_, stile_dst_;
  DBuf<double> rdg_;       // 1/U_jj of the factor
  DBuf<double> mk_, mq_, mt_, mX_, mobs_pt_, mobs_err_, mred_;
  HostIo io_;   // ReprojectMap's uploads and downloads (hostio.h)
  double range_b_ = 4.0, fd_target_ = 150.0, fd_b2_ = 225.0;
  // timing
  bool timing_ = false;
  struct KTimer {
    std::string name;
    std::vector<hipEvent_t> ev;  // pairs
    double total_ms = 0.0;
    int count = 0;
  };
  std::vector<KTimer> timers_;
  void TimedLaunchBegin(int id);
  void LaunchCholTiles(bool stamp, dim3 grid, const Dev& d, int flags);
  void TimedLaunchEnd(int id);
  void TimedLaunchBegin(int id, hipStream_t s);
  void TimedLaunchEnd(int id, hipStream_t s);
  void CollectTimes();
  Dev MakeDev();
  void AllReduceSum(double* buf, size_t n);
};

}  // namespace sg

#endif  // SG_BA_SOLVER_H_
