// ba_solver.hip — host driver of the MI355X-native Levenberg-Marquardt bundle adjustment (the reference's
// Slam::Run, slam.cpp:482-521, which hands the problem to Ceres 1.8 with SPARSE_SCHUR; restated on gfx950):
// problem load (the lists planned by ba_plan.cpp uploaded, the buffers sized, the structure-only incremental
// path), the per-iteration kernel chain and the host polls.  The kernels are in the family translation units listed in
// ba_launch.h; this file launches them through ba_launch.h's launchers and keeps only a few utility kernels
// (copies, buffer resets, the state hand-off, the solution download).
//
// One LM iteration = the kernel chain below, enqueued without host synchronisation; the accept/reject
// decision, trust-region update and termination tests run on the device, so a solve is a stream of identical
// iterations the host only polls for completion.  The default chain (one GPU, speculative linearization):
//   k_schur        (+ one workgroup: the camera finalize pass, FrameDistance / cost / gradient / LM diagonal)
//                  whitened point Jacobians, -E E^T into the segment's window tiles on the matrix cores
//   k_S_reduce     fixed-order reduce of the window tiles + blockdiag(U) + FrameDistance + damping -> S, rhs
//   k_chol_tiles   dissected tiled band Cholesky of S, back substitution, candidate poses
//   k_update_lin   point back substitution, model and candidate cost, and the linearization at the candidate
//   k_cam_reduce   the candidate's camera partials and update scalars reduced, and the LM decision (mode 2)
// Landmark shards add the exchanges of DESIGN.md 5 (pack, all-reduce, unpack) and the separate decision; the chain
// of every regime is planned in ba_chain.cpp.
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <thread>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <numeric>

#include "ba_solver.h"
#include "ba_device.h"
#include "ba_launch.h"
#include "comm.h"
#include "stager.h"

namespace sg {

// Word copy (8-byte words, grid-stride) between device and mapped host memory.
__global__ __launch_bounds__(256) void k_copy_u64(const unsigned long long* __restrict__ src,
                                                  unsigned long long* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}

// ================================================================================================
// Host driver

enum KernelId { kKLin = 0, kKCamReduce, kKCamFinal, kKSchur, kKSReduce, kKChol, kKPointUpd, kKUpdRed, kKDecide,
                kKXchg, kKNum };
static const char* kKernelNames[kKNum] = {"linearize", "cam_reduce", "cam_finalize", "schur", "S_reduce",
                                          "cholesky", "point_update", "upd_reduce", "decide", "exchange"};

void BaSolver::LaunchCholTiles(bool stamp, dim3 grid, const Dev& d, int flags) {
  // bordered: the frame band ends follow the arrowhead's panel ends in work_i_
  const int32_t* pj = (const int32_t*)work_i_.ptr + (chol_.border ? (n_ + kCholNb - 1) / kCholNb : 0);
  if (chol_.border) flags |= 8;
  LaunchCholTilesK(stamp, grid, chol_.tile_lds, stream_, d, pj, Wg_.ptr, tflag_.ptr, chol_.nd, flags | (chol_.ns << 8));
  if (chol_.border) {
    const int ntf = (6 * NB_ + kCholNb - 1) / kCholNb;
    LaunchCholBorderK(chol_.border_flags, border_lds_doubles(ntf, chol_.border_flags, F_, D_, n_) * sizeof(double), stream_, d,
                      Wg_.ptr);
  }
}

static RunKnobs ReadRunKnobs();   // (beside ReadLoadKnobs, below)

BaSolver::BaSolver(const sg_device_options& dev) : dev_(dev), knobs_(ReadRunKnobs()) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw Error(SG_ENODEV, "no HIP device available");
  SG_REQUIRE(dev.device >= 0 && dev.device < ndev, SG_ENODEV, "device ordinal out of range");
  SG_REQUIRE(dev.precision == 0, SG_EINVAL,
             "sg_device_options.precision: only 0 (fp64, the reference's arithmetic) is implemented");
  SG_HIP_CHECK(hipSetDevice(dev.device));
  SG_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev.device) == hipSuccess && prop.multiProcessorCount > 0)
      ncu_ = prop.multiProcessorCount;
  }
  stager_.reset(new Stager());
  CholSetAttributes(&tile_lds_set_, &gchol_lds_max_, &border_lds_max_);
  st_.Resize(1);
  timers_.resize(kKNum);
  for (int i = 0; i < kKNum; ++i) timers_[i].name = kKernelNames[i];
}

BaSolver::~BaSolver() {
  for (auto& t : timers_)
    for (auto e : t.ev) (void)hipEventDestroy(e);
  if (ev_wait_) (void)hipEventDestroy(ev_wait_);
  if (ev_idle_) (void)hipEventDestroy(ev_idle_);
  if (ev_idle_prev_) (void)hipEventDestroy(ev_idle_prev_);
  if (stream_) (void)hipStreamDestroy(stream_);
}

void BaSolver::UniqueId(void* id128) { RcclComm::UniqueId(id128); }

void BaSolver::CommInit(const void* id128, int nranks, int rank) {
  SG_REQUIRE(!loaded_, SG_EINVAL, "sg_ba_comm_init must precede sg_ba_load (exchange buffers are sized by it)");
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  comm_.reset(new RcclComm(id128, nranks, rank));
  dev_.nranks = nranks;
  dev_.rank = rank;
}

void BaSolver::CommInitLocal(std::shared_ptr<LocalGroup> g, int rank) {
  SG_REQUIRE(!loaded_, SG_EINVAL, "sg_ba_comm_init_local must precede sg_ba_load");
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  comm_.reset(new LocalComm(std::move(g), rank));
  dev_.nranks = comm_->nranks();
  dev_.rank = rank;
}

void BaSolver::CommInitHost(int nranks, int rank, int (*fn)(double*, long long, int, void*), void* user) {
  SG_REQUIRE(!loaded_, SG_EINVAL, "sg_ba_comm_init_host must precede sg_ba_load");
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  comm_.reset(new HostComm(nranks, rank, fn, user));
  dev_.nranks = comm_->nranks();
  dev_.rank = rank;
}

int BaSolver::nranks() const { return comm_ ? comm_->nranks() : 1; }

void BaSolver::AllReduceSum(double* buf, size_t n) {
  if (comm_ && (comm_->nranks() > 1 || knobs_.comm_force)) {
    comm_->AllReduceSum(buf, n, stream_);
    ++nallreduce_;
  }
}

__global__ __launch_bounds__(256) void k_fill_obs_pnt(const int32_t* __restrict__ poff, int32_t* __restrict__ obs_pnt,
                                                      int P) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  for (int o = poff[i]; o < poff[i + 1]; ++o) obs_pnt[o] = i;
}

// The knobs of a full load, read at every one (A/B switches and tests: DESIGN.md).
static LoadKnobs ReadLoadKnobs() {
  auto is = [](const char* name, int v) { return getenv(name) && atoi(getenv(name)) == v; };
  LoadKnobs k;
  if (const char* e = getenv("SG_LIN_WAVES")) k.lin_waves = atoi(e) == 2 ? 2 : 1;
  k.chol_gstage = !is("SG_CHOL_GSTAGE", 0);
  k.chol_window = getenv("SG_CHOL_WINDOW") != nullptr;
  k.chol_border = !is("SG_CHOL_BORDER", 0);
  k.chol_split = !is("SG_CHOL_SPLIT", 0);
  k.chol_sep7 = is("SG_CHOL_SEP", kTB - 1);
  k.stamp = getenv("SG_STAMP") && getenv("SG_STAMP")[0] == '1';
  if (const char* e = getenv("SG_WT_STORES")) k.wt_stores = atoi(e) & (kWtJ | kWtCam | kWtSchur);
  return k;
}

// The knobs of the iteration chain (ba_chain.h), read once when the solver is created: a caller sets the switches,
// then creates its handle.
static RunKnobs ReadRunKnobs() {
  auto is = [](const char* name, int v) { return getenv(name) && atoi(getenv(name)) == v; };
  auto str = [](const char* name) { return std::string(getenv(name) ? getenv(name) : ""); };
  RunKnobs k;
  k.spec = !is("SG_SPEC", 0);
  if (getenv("SG_XCHG_MERGE")) k.merge = str("SG_XCHG_MERGE") == "force" ? 2 : !is("SG_XCHG_MERGE", 0);
  k.pack_force = getenv("SG_PACK_S") != nullptr;
  k.comm_force = is("SG_COMM_FORCE", 1);
  k.chol_zpre = !is("SG_CHOL_ZPRE", 0);
  k.chol_stile = !is("SG_CHOL_STILE", 0);
  k.chol_force_tmo = getenv("SG_CHOL_FORCE_TIMEOUT") && !is("SG_CHOL_FORCE_TIMEOUT", 0);
  k.chol_delay = str("SG_CHOL_DELAY") == "bottom" ? 64 : str("SG_CHOL_DELAY") == "top" ? 128 : 0;
  return k;
}

// SG_HOST_TIMING: the device's share of a full load (the marks Load set), against the host's wall time.
std::string BaSolver::LoadDeviceTimes(std::chrono::steady_clock::time_point load_t0, bool idle_valid_prev,
                                      double idle_gap_host) {
  std::string log;
  float a = 0, b = 0, c = 0;
  (void)hipEventElapsedTime(&a, dev_marks_[0], dev_marks_[1]);
  (void)hipEventElapsedTime(&b, dev_marks_[1], dev_marks_[2]);
  (void)hipEventElapsedTime(&c, dev_marks_[2], dev_marks_[3]);
  float e = 0;
  (void)hipEventElapsedTime(&e, dev_marks_[4], dev_marks_[3]);
  const double hw = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - load_t0).count();
  char buf[320];
  snprintf(buf, sizeof(buf), " [device: batch1..batch2 %.2f, scatter2 %.2f, reset %.2f; load start..reset: device "
           "%.2f, host %.2f]", a, b, c, e, hw);
  log += buf;
  if (idle_valid_prev) {
    float g = 0;
    const hipError_t ge = hipEventElapsedTime(&g, ev_idle_prev_, dev_marks_[4]);
    snprintf(buf, sizeof(buf), " [last idle..load start: device %.2f (%d), host %.2f]", g, (int)ge, idle_gap_host);
    log += buf;
  }
  snprintf(buf, sizeof(buf), " (staged %.2f MB; device allocations so far %ld)", stager_->staged_bytes() / 1e6,
           g_dbuf_allocs.load());
  log += buf;
  return log;
}

// What the device solver's packed indices hold (beyond ValidateProblem's checks of the problem itself).
static void ValidateDeviceLimits(const sg_problem& p, int nranks) {
  SG_REQUIRE(!p.cameras_free || (p.num_cameras <= kMaxIntrCams && nranks == 1), SG_EINVAL,
             "free intrinsics: at most 4 cameras, on one rank (landmark shards keep the intrinsics constant)");
  SG_REQUIRE(p.num_cameras <= 0xff, SG_EINVAL, "too many cameras for the device solver");
  int nfree = 0;
  for (int f = 0; f < p.num_frames; ++f) nfree += (p.frame_rot_free[f] || p.frame_trans_free[f]) ? 1 : 0;
  SG_REQUIRE(nfree < 0xffff, SG_EINVAL, "too many free frames for the device solver");
  std::vector<int32_t> cnt(p.num_points, 0);
  for (int o = 0; o < p.num_obs; ++o)
    SG_REQUIRE(++cnt[p.obs_point[o]] < 65536, SG_EINVAL, "a point has 65536 or more observations");
}

void BaSolver::Load(const sg_problem& p) {
  static const bool host_timing = getenv("SG_HOST_TIMING") != nullptr;   // development aid: phase times
  auto lt0 = std::chrono::steady_clock::now();
  std::string lap_log;
  auto lap = [&](const char* what) {
    if (!host_timing) return;
    const auto t = std::chrono::steady_clock::now();
    char buf[96];
    snprintf(buf, sizeof(buf), " %s %.2f", what, std::chrono::duration<double, std::milli>(t - lt0).count());
    lap_log += buf;
    lt0 = t;
  };
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  // a device mark at the load's start, with its host time: the GPU time from here to the last mark against the
  // host's wall time tells a late device (its queue started late) from a late host (the waiting thread)
  auto load_t0 = std::chrono::steady_clock::now();
  const bool idle_valid_prev = idle_valid_;
  const double idle_gap_host =
      idle_valid_ ? std::chrono::duration<double, std::milli>(load_t0 - idle_host_).count() : 0.0;
  std::swap(ev_idle_, ev_idle_prev_);   // (this load's own waits re-mark ev_idle_)
  if (host_timing) DevMark(stream_, 4);
  {
    // Everything that can reject this rank's problem runs before the first collective, and the verdict rides
    // in that collective (2: some rank's problem is invalid), so that all ranks fail together instead of
    // leaving the others blocked in an all-reduce.
    int vcode = SG_OK;
    std::string verr;
    try {
      ValidateProblem(&p);
      ValidateDeviceLimits(p, nranks());
    } catch (const Error& e) {
      vcode = e.code;
      verr = e.what();
    }
    // incremental update: every rank must take the same path (the full path has a load-time all-reduce)
    double changed = vcode != SG_OK ? 2.0 : (loaded_ && SameStructure(p)) ? 0.0 : 1.0;
    if (comm_ && (comm_->nranks() > 1 || knobs_.comm_force)) {
      DBuf<double> flag;
      flag.Upload(std::vector<double>{changed}, stream_);
      comm_->AllReduceMax(flag.ptr, 1, stream_);
      SG_HIP_CHECK(hipMemcpyAsync(&changed, flag.ptr, sizeof(double), hipMemcpyDeviceToHost, stream_));
      SG_HIP_CHECK(hipStreamSynchronize(stream_));
    }
    if (vcode != SG_OK) throw Error(vcode, verr);
    if (changed == 2.0) throw Error(SG_EINVAL, "another landmark shard's problem failed validation");
    if (changed == 0.0) {
      LoadValues(p);
      lap("values");
      if (host_timing) fprintf(stderr, "[sg] Load phases (ms):%s\n", lap_log.c_str());
      return;
    }
  }
  // Full path: the structure and every device list are rebuilt below.  Until that completes, this solver
  // holds no usable problem: a failure part way (a device allocation, a hipFuncSetAttribute) must not leave
  // the previous problem's structure key matching a later load's value-only path.
  loaded_ = false;
  began_ = false;
  skey_ = StructKey{};
  stager_->Clear();
  F_ = p.num_frames;
  P_ = p.num_points;
  M_ = p.num_obs;
  D_ = p.num_dist;
  ncam_ = p.num_cameras;
  range_b_ = p.range * p.range;
  fd_target_ = p.dist_target;
  fd_b2_ = p.dist_range * p.dist_range;
  stab_b_ = p.stab_range * p.stab_range;
  const LoadKnobs knobs = ReadLoadKnobs();
  // The lists are planned on the host alone (ba_plan.h); this function uploads them and sizes the buffers.
  Order ord;
  PlanBlocks(p, &ord);
  NB_ = ord.NB;
  nk_ = ord.nk;
  n_ = ord.n;
  lap("blocks");
  PlanPointOrder(p, &ord);
  lap("point-order");
  PlanObservations(p, &ord);
  lap("obs-csr");
  // upload batch 1 — poses, intrinsics, points (current slot; the candidate slot is a device copy) and the
  // observation arrays: its pinned copy and DMA overlap the host's work-list construction below (stager.h)
  hipStream_t s = stream_;
  Stager& stg = *stager_;
  stg.ResetBytes();
  stg.AddInto(k_, std::max<size_t>(14 * (size_t)ncam_, 1),
              ncam_ > 0 ? std::vector<double>(p.k, p.k + 7 * ncam_) : std::vector<double>{0.0});
  stg.AddInto(q_, 8 * (size_t)F_, std::vector<double>(p.q, p.q + 4 * F_));
  stg.AddInto(t_, 6 * (size_t)F_, std::vector<double>(p.t, p.t + 3 * F_));
  stg.AddInto(X_, 8 * (size_t)P_, ord.X);
  stg.Add(frame_cam_, std::vector<int32_t>(p.frame_camera, p.frame_camera + F_));
  stg.Add(frame_block_, ord.frame_block);
  stg.Add(rot_free_, std::vector<uint8_t>(p.frame_rot_free, p.frame_rot_free + F_));
  stg.Add(trans_free_, std::vector<uint8_t>(p.frame_trans_free, p.frame_trans_free + F_));
  stg.Add(pfree_, ord.pfree);
  stg.Add(poff_, ord.poff);
  stg.Add(obs_pt_, ord.obs_pt);
  stg.Add(obs_frame_, ord.obs_frame);
  stg.Add(obs_fixed_, ord.obs_fixed);
  stg.Add(obs_meta_, ord.obs_meta);
  if (host_timing) DevMark(s, 0);
  stg.Flush(s);
  {
    auto dup = [&](double* base, size_t half) {   // candidate slot = current slot
      if (half)   // a kernel, not a copy-engine hipMemcpyAsync (see hostmirror.h)
        hipLaunchKernelGGL(k_copy_u64, dim3((unsigned)std::min<size_t>(256, (half + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const unsigned long long*>(base),
                           reinterpret_cast<unsigned long long*>(base + half), half);
    };
    dup(k_.ptr, 7 * (size_t)ncam_);
    dup(q_.ptr, 4 * (size_t)F_);
    dup(t_.ptr, 3 * (size_t)F_);
    dup(X_.ptr, 4 * (size_t)P_);
    // the point of every observation (device order) from the CSR, on the device
    obs_pnt_.Resize(std::max(M_, 1));
    if (P_ > 0)
      hipLaunchKernelGGL(k_fill_obs_pnt, dim3((P_ + 255) / 256), dim3(256), 0, s, (const int32_t*)poff_.ptr,
                         obs_pnt_.ptr, P_);
    SG_HIP_CHECK(hipGetLastError());
  }
  lap("upload-1");
  WorkLists wl;
  PlanSweep(ord, ncu_, knobs.lin_waves, &wl);
  lap("lin-lists");
  PlanSchur(ord, ncu_, &wl);
  lap("segments");
  PlanReduceLists(ord, &wl);
  lap("reduce-lists");
  PlanFrameDistance(p, ord, &wl);
  PlanIntrLists(ord, &wl);
  lap("fd");
  PlanLoBlk(ord, &wl);
  // Landmark shards: S is summed over every rank's points, so each rank must factor it with the envelope of
  // the whole problem (the union of the shards' envelopes), not of its own points.  One max all-reduce of
  // -lo(J) at load time.
  if (comm_ && (comm_->nranks() > 1 || knobs_.comm_force) && NB_ > 0) {
    std::vector<double> neg(NB_);
    for (int b = 0; b < NB_; ++b) neg[b] = -(double)wl.lo_blk[b];
    DBuf<double> env;
    env.Upload(neg, stream_);
    comm_->AllReduceMax(env.ptr, (size_t)NB_, stream_);
    SG_HIP_CHECK(hipMemcpyAsync(neg.data(), env.ptr, NB_ * sizeof(double), hipMemcpyDeviceToHost, stream_));
    SG_HIP_CHECK(hipStreamSynchronize(stream_));
    for (int b = 0; b < NB_; ++b) wl.lo_blk[b] = (int)(-neg[b]);
  }
  const Envelope env = PlanEnvelope(ord, wl.lo_blk, wl.segs, wl.nseg);
  chol_ = PlanChol(ord, env, CholGrants{tile_lds_set_, gchol_lds_max_, border_lds_max_}, knobs);
  wk_ = wl;    // (the counts: the lists live on the device only)
  env_ = env;
  lap("envelope");
  stg.Add(pack_off_, env.pack_off);
  // + the merged exchange's tail (k_cam_finalize modes 1, 2)
  ntail_ = 2 * (size_t)6 * NB_ + kXNum + nranks() + 1;
  Spk_.Resize(env.npack + ntail_);
  if (chol_.wg_size) {   // (zeroed and its constants set on the device by ResetState: no host fill, no staged zeros)
    Wg_.Resize(chol_.wg_size);
    stg.Add(tflag_, std::vector<int32_t>(2, 0));
  }
  // upload batch 2 — the work lists: one pinned staging copy and one scatter launch (stager.h)
  stg.Add(lchunks_d_, wl.lchunks);
  stg.Add(lrounds_d_, wl.lrounds);
  stg.Add(segs_, wl.segs);
  stg.Add(sbatch_, wl.sbatch);
  stg.Add(wsegs_, wl.wsegs);
  stg.Add(pinfo_, wl.pinfo);
  stg.Add(pmx_, wl.pmx);
  stg.Add(cells_, wl.cells);
  stg.Add(cell_obs_, wl.cell_obs);
  stg.Add(stile_, env.stile);
  {   // the tiles' slots in St, then the bottom workgroup's band ends (one list: Dev::stile_dst)
    StilePlan sp = PlanStile(env, chol_);
    sp.dst.insert(sp.dst.end(), sp.tend_rev.begin(), sp.tend_rev.end());
    stg.Add(stile_dst_, sp.dst);
  }
  stg.Add(pairs_, wl.pairs);
  seg_fail_.Resize(std::max(wl.nseg + wl.nwide, 1));
  stg.Add(cam_loff_, wl.cam_loff);
  stg.Add(cam_lidx_, wl.cam_lidx);
  stg.Add(s_loff_, env.s_loff);
  stg.Add(s_lidx_, env.s_lidx);
  stg.Add(r_loff_, wl.r_loff);
  stg.Add(r_lidx_, wl.r_lidx);
  stg.Add(fd_a_, wl.fd_a);
  stg.Add(fd_b_, wl.fd_b);
  stg.Add(fd_boff_, wl.fd_boff);
  stg.Add(fd_bidx_, wl.fd_bidx);
  stg.Add(work_i_, env.panel_jmax);
  stg.Add(fd_pair_, wl.fd_pair);
  rdg_.Resize((size_t)std::max(n_, 1) + kCholNb);   // + padding rows of the last panel
  // the linearization's buffers hold two slots (current point, k_update_lin's candidate)
  jslot_ = (size_t)((std::max(M_, 1) + 63) & ~63) * kJStride;   // whole 64-observation blocks (jidx2)
  J_.Resize(2 * jslot_);
  V_.Resize(2 * 10 * (size_t)std::max(P_, 1));
  g_.Resize(2 * 4 * (size_t)std::max(P_, 1));
  scale_p_.Resize(4 * (size_t)std::max(P_, 1));
  diag_p_.Resize(4 * (size_t)std::max(P_, 1));
  Vinv_.Resize(10 * (size_t)std::max(P_, 1));
  tp_.Resize(4 * (size_t)std::max(P_, 1));
  const size_t nn = std::max(n_, 1);
  scale_c_.Resize(nn);
  diag_c_.Resize(nn);
  camdiag_.Resize(nn);
  camg_.Resize(nn);
  cslot_ = std::max(wl.lcam_off, 1);
  cam_slab_.Resize(2 * cslot_);
  lin_scal_.Resize(2 * (size_t)std::max(wl.nlin, 1) * kNScal);
  S_slab_.Resize(std::max(wl.s_off, 1));
  chunk_scal_.Resize((size_t)std::max(wl.npu, 1) * kNScal);
  stg.Add(pu_units_, wl.pu_units);
  if (nk_) {
    stg.Add(intr_boff_, wl.intr_boff);
    stg.Add(intr_bidx_, wl.intr_bidx);
  }
  point_perm_ = std::move(ord.point_perm);
  obs_perm_ = std::move(ord.obs_perm);
  if (host_timing) DevMark(s, 1);
  stg.Flush(s);
  if (host_timing) DevMark(s, 2);
  lap("flush");
  cam_wide_.Resize(2 * (size_t)std::max(NB_, 1) * kCamV);
  S_wide_.Resize(nn * nn);
  zpre_.Resize(257);
  xchg_cam_.Resize(3 * ((size_t)NB_ * kCamV + kXNum + nranks()));   // summed | this rank's | candidate
  S_.Resize(nn * nn + nn + 2);   // S, then the rhs partial xc (one all-reduce covers both), then {0, 1}
  rhs_.Resize(nn);
  xchg_upd_.Resize(kUNum);
  xchg_chol_.Resize(kCNum);
  work_.Resize(nn);
  fd_r_.Resize(std::max(D_, 1));
  fd_J_.Resize(6 * (size_t)std::max(D_, 1));
  fd_D_.Resize(9 * (size_t)std::max(NB_, 1));
  fd_X_.Resize(9 * (size_t)std::max(D_, 1));
  if (nk_) {
    Jk_.Resize(14 * (size_t)std::max(M_, 1));
    KU_.Resize(nn * nk_);
    kst_.Resize(56 * (size_t)ncam_);
    Yk_.Resize(28 * (size_t)std::max(P_, 1) * ncam_);
    kpart_.Resize((size_t)(NB_ + 1) * ncam_ * 42);
  }
  wt_stores_ = knobs.wt_stores;
  stamp_on_ = knobs.stamp;
  if (stamp_on_) stamps_.Resize(kStampWords);
  lap("resize");
  ResetState(s);
  if (host_timing) DevMark(s, 3);
  lap("reset");
  WaitStream(s);
  lap("uploads");
  if (host_timing) lap_log += LoadDeviceTimes(load_t0, idle_valid_prev, idle_gap_host);
  SaveStructure(p);
  full_loads_++;
  chol_stile_last_ = false;
  if (host_timing) {
    SG_HIP_CHECK(hipStreamSynchronize(stream_));
    lap("sync");
    fprintf(stderr, "[sg] Load phases (ms):%s\n", lap_log.c_str());
  }
  loaded_ = true;
  began_ = false;
  pending_decision_ = false;
}

void BaSolver::Reserve(int F, int P, int M) {
  SG_REQUIRE(F >= 0 && P >= 0 && M >= 0, SG_EINVAL, "negative reservation");
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  const size_t f = std::max(F, 1), pp = std::max(P, 1), m = std::max(M, 1);
  bool moved = false;
  // per observation (device order records, the Jacobian rows, the Schur cells)
  moved |= J_.Reserve(2 * ((m + 63) & ~(size_t)63) * kJStride);
  moved |= obs_pt_.Reserve(2 * m);
  moved |= obs_frame_.Reserve(m);
  moved |= obs_fixed_.Reserve(m);
  moved |= obs_meta_.Reserve(m);
  moved |= obs_pnt_.Reserve(m);
  moved |= cells_.Reserve(4 * m);
  moved |= cell_obs_.Reserve(m);
  // per point
  moved |= X_.Reserve(8 * pp);
  moved |= V_.Reserve(2 * 10 * pp);
  moved |= Vinv_.Reserve(10 * pp);
  moved |= g_.Reserve(2 * 4 * pp);
  moved |= tp_.Reserve(4 * pp);
  moved |= scale_p_.Reserve(4 * pp);
  moved |= diag_p_.Reserve(4 * pp);
  moved |= pfree_.Reserve(pp);
  moved |= poff_.Reserve(pp + 1);
  moved |= pinfo_.Reserve(2 * pp);
  moved |= pmx_.Reserve(4 * pp);
  // per frame
  moved |= q_.Reserve(8 * f);
  moved |= t_.Reserve(6 * f);
  moved |= frame_cam_.Reserve(f);
  moved |= frame_block_.Reserve(f);
  moved |= rot_free_.Reserve(f);
  moved |= trans_free_.Reserve(f);
  // the pinned staging buffer and its device copy: about 51 B per observation, 93 B per point, and per frame
  // the pose slots, the FrameDistance pair table (NB^2) and the Cholesky's W tiles (2 * 8 tiles per 16 columns)
  moved |= stager_->ReserveBytes(64 * m + 128 * pp + 16384 * f + 4 * f * f + (1u << 20));
  if (moved) {   // the buffers of the loaded structure are gone: the next Load rebuilds everything
    loaded_ = false;
    began_ = false;
    skey_ = StructKey{};
  }
}

bool BaSolver::SameStructure(const sg_problem& p) const {
  const StructKey& k = skey_;
  if (p.num_cameras != k.ncam || (p.cameras_free != 0) != (k.cams_free != 0) || p.num_frames != k.F ||
      p.num_points != k.P || p.num_obs != k.M || p.num_dist != k.D)
    return false;
  auto same = [](const auto* a, const auto& v) {
    return v.empty() || std::memcmp(a, v.data(), v.size() * sizeof(v[0])) == 0;
  };
  return same(p.frame_camera, k.frame_camera) && same(p.frame_rot_free, k.rot_free) &&
         same(p.frame_trans_free, k.trans_free) && same(p.point_free, k.point_free) &&
         same(p.obs_frame, k.obs_frame) && same(p.obs_point, k.obs_point) && same(p.dist_frame, k.dist_frame) &&
         same(p.dist_prev, k.dist_prev);
}

void BaSolver::SaveStructure(const sg_problem& p) {
  StructKey& k = skey_;
  k.ncam = p.num_cameras;
  k.cams_free = p.cameras_free != 0;
  k.F = p.num_frames;
  k.P = p.num_points;
  k.M = p.num_obs;
  k.D = p.num_dist;
  k.frame_camera.assign(p.frame_camera, p.frame_camera + k.F);
  k.rot_free.assign(p.frame_rot_free, p.frame_rot_free + k.F);
  k.trans_free.assign(p.frame_trans_free, p.frame_trans_free + k.F);
  k.point_free.assign(p.point_free, p.point_free + k.P);
  k.obs_frame.assign(p.obs_frame, p.obs_frame + k.M);
  k.obs_point.assign(p.obs_point, p.obs_point + k.M);
  k.dist_frame.assign(p.dist_frame, p.dist_frame + k.D);
  k.dist_prev.assign(p.dist_prev, p.dist_prev + k.D);
}

// LM state and accumulators a fresh solve starts from (zeroed on every Load)
// Zero a few device buffers and set the tiled Cholesky's {0, 1} constants (after S and its rhs) in one launch
// (hipMemsetAsync / a pageable hipMemcpyAsync would go through the copy engine).
constexpr int kZeroBufs = 9;
struct ZeroList {
  double* p[kZeroBufs];
  size_t n[kZeroBufs];   // doubles
  double* c01[2];        // two doubles each: {0, 1}
};
__global__ __launch_bounds__(256) void k_reset_buffers(ZeroList z) {
  for (int b = 0; b < kZeroBufs; ++b) {
    double* p = z.p[b];
    const size_t n = z.n[b];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
      p[i] = 0.0;
  }
  if (blockIdx.x == 0 && threadIdx.x < 2 && z.c01[threadIdx.x]) {
    z.c01[threadIdx.x][0] = 0.0;
    z.c01[threadIdx.x][1] = 1.0;
  }
}

void BaSolver::ResetState(hipStream_t s) {
  // LmState (slot 0 current, nothing pending: evaluate() may run before begin()), the accumulators, S; one
  // launch, no copy engine (hostmirror.h)
  ZeroList z{};
  auto put = [&](int i, void* ptr, size_t bytes) {
    z.p[i] = static_cast<double*>(ptr);
    z.n[i] = ptr ? bytes / 8 : 0;
  };
  static_assert(sizeof(LmState) % 8 == 0, "LmState is zeroed in 8-byte words");
  put(0, st_.ptr, st_.size * sizeof(LmState));
  put(1, lin_scal_.ptr, lin_scal_.size * sizeof(double));
  put(2, seg_fail_.ptr, seg_fail_.size * sizeof(*seg_fail_.ptr));
  put(3, cam_wide_.ptr, cam_wide_.size * sizeof(double));
  put(4, S_wide_.ptr, S_wide_.size * sizeof(double));
  put(5, rhs_.ptr, rhs_.size * sizeof(double));
  put(6, chunk_scal_.ptr, chunk_scal_.size * sizeof(double));
  put(7, S_.ptr, (S_.size - 2) * sizeof(double));
  z.c01[0] = S_.ptr + S_.size - 2;   // k_chol_tiles: padding entries of the last tile
  if (chol_.tiles && Wg_.size >= 2) {   // its W tiles, z', separator terms, then its own {0, 1}
    put(8, Wg_.ptr, (Wg_.size - 2) * sizeof(double));
    z.c01[1] = Wg_.ptr + Wg_.size - 2;
  }
  size_t mx = 0;
  for (int i = 0; i < kZeroBufs; ++i) mx = std::max(mx, z.n[i]);
  const unsigned g = (unsigned)std::min<size_t>(512, std::max<size_t>(1, (mx + 255) / 256));
  hipLaunchKernelGGL(k_reset_buffers, dim3(g), dim3(256), 0, s, z);
  SG_HIP_CHECK(hipGetLastError());
  if (stamp_on_) stamps_.Zero(s);
}

// Same structure as the last Load: new values (poses, intrinsics, points, observed pixels, loss ranges) in
// the device order of that Load; every index list and the Cholesky envelope stay.
void BaSolver::LoadValues(const sg_problem& p) {
  range_b_ = p.range * p.range;
  fd_target_ = p.dist_target;
  fd_b2_ = p.dist_range * p.dist_range;
  stab_b_ = p.stab_range * p.stab_range;
  hipStream_t s = stream_;
  std::vector<double> k2(14 * (size_t)ncam_), q2(8 * (size_t)F_), t2(6 * (size_t)F_), X2(8 * (size_t)P_),
      obs_pt(2 * (size_t)M_);
  for (int c = 0; c < 7 * ncam_; ++c) k2[c] = k2[c + 7 * ncam_] = p.k[c];
  for (int i = 0; i < 4 * F_; ++i) q2[i] = q2[i + 4 * F_] = p.q[i];
  for (int i = 0; i < 3 * F_; ++i) t2[i] = t2[i + 3 * F_] = p.t[i];
  for (int i = 0; i < P_; ++i) {
    const int pt = point_perm_[i];
    for (int a = 0; a < 4; ++a) X2[4 * i + a] = X2[4 * (i + P_) + a] = p.X[4 * pt + a];
  }
  for (int o = 0; o < M_; ++o) {
    const int src = obs_perm_[o];
    obs_pt[2 * o] = p.obs_pt[2 * src];
    obs_pt[2 * o + 1] = p.obs_pt[2 * src + 1];
  }
  k_.Upload(k2.empty() ? std::vector<double>{0.0} : k2, s);
  q_.Upload(q2, s);
  t_.Upload(t2, s);
  X_.Upload(X2, s);
  obs_pt_.Upload(obs_pt, s);
  ResetState(s);
  SG_HIP_CHECK(hipStreamSynchronize(s));
  value_loads_++;
  loaded_ = true;
  began_ = false;
  pending_decision_ = false;
}

Dev BaSolver::MakeDev() {
  Dev d{};
  d.st = st_.ptr;
  d.k[0] = k_.ptr;
  d.k[1] = k_.ptr + 7 * (size_t)ncam_;
  d.nk = nk_;
  d.kc0 = 6 * NB_;
  d.ncam = ncam_;
  d.Jk = Jk_.ptr;
  d.KU = KU_.ptr;
  d.kst = kst_.ptr;
  d.Yk = Yk_.ptr;
  d.kpart = kpart_.ptr;
  d.intr_boff = intr_boff_.ptr;
  d.intr_bidx = intr_bidx_.ptr;
  d.stab_b = stab_b_;
  d.stab_inv_b = 1.0 / stab_b_;
  d.q[0] = q_.ptr;
  d.q[1] = q_.ptr + 4 * (size_t)F_;
  d.t[0] = t_.ptr;
  d.t[1] = t_.ptr + 3 * (size_t)F_;
  d.frame_cam = frame_cam_.ptr;
  d.frame_block = frame_block_.ptr;
  d.rot_free = rot_free_.ptr;
  d.trans_free = trans_free_.ptr;
  d.F = F_;
  d.NB = NB_;
  d.n = n_;
  d.X[0] = X_.ptr;
  d.X[1] = X_.ptr + 4 * (size_t)P_;
  d.pfree = pfree_.ptr;
  d.poff = poff_.ptr;
  d.P = P_;
  d.M = M_;
  d.obs_pt = obs_pt_.ptr;
  d.obs_frame = obs_frame_.ptr;
  d.obs_fixed = obs_fixed_.ptr;
  d.obs_meta = obs_meta_.ptr;
  d.b = range_b_;
  d.inv_b = 1.0 / range_b_;
  d.D = D_;
  d.fd_a = fd_a_.ptr;
  d.fd_b = fd_b_.ptr;
  d.fd_boff = fd_boff_.ptr;
  d.fd_bidx = fd_bidx_.ptr;
  d.fd_target = fd_target_;
  d.fd_b2 = fd_b2_;
  d.fd_inv_b2 = 1.0 / fd_b2_;
  d.fd_r = fd_r_.ptr;
  d.fd_J = fd_J_.ptr;
  d.fd_D = fd_D_.ptr;
  d.fd_X = fd_X_.ptr;
  {
    const size_t pp = std::max(P_, 1);
    for (int sl = 0; sl < 2; ++sl) {
      d.J[sl] = J_.ptr + sl * jslot_;
      d.V[sl] = V_.ptr + sl * 10 * pp;
      d.g[sl] = g_.ptr + sl * 4 * pp;
      d.cam_slab[sl] = cam_slab_.ptr + sl * cslot_;
      d.cam_wide[sl] = cam_wide_.ptr + sl * (size_t)std::max(NB_, 1) * kCamV;
      d.lin_scal[sl] = lin_scal_.ptr + sl * (size_t)std::max(wk_.nlin, 1) * kNScal;
    }
  }
  d.spec = knobs_.spec ? 1 : 0;
  d.scale_p = scale_p_.ptr;
  d.diag_p = diag_p_.ptr;
  d.Vinv = Vinv_.ptr;
  d.tp = tp_.ptr;
  d.scale_c = scale_c_.ptr;
  d.diag_c = diag_c_.ptr;
  d.camdiag = camdiag_.ptr;
  d.camg = camg_.ptr;
  d.cam_loff = cam_loff_.ptr;
  d.cam_lidx = cam_lidx_.ptr;
  d.s_loff = s_loff_.ptr;
  d.s_lidx = s_lidx_.ptr;
  d.r_loff = r_loff_.ptr;
  d.r_lidx = r_lidx_.ptr;
  d.s_lstride = env_.s_lstride;
  d.r_lstride = wk_.r_lstride;
  d.S_slab = S_slab_.ptr;
  d.chunk_scal = chunk_scal_.ptr;
  d.S_wide = S_wide_.ptr;
  d.zpre = zpre_.ptr;
  d.xchg_cam = xchg_cam_.ptr;
  d.xcam_loc = xchg_cam_.ptr + (size_t)NB_ * kCamV + kXNum + nranks();
  d.xchg_cand = xchg_cam_.ptr + 2 * ((size_t)NB_ * kCamV + kXNum + nranks());
  d.xtail = Spk_.ptr + env_.npack;
  d.rank = comm_ ? comm_->rank() : 0;
  d.nranks = nranks();
  d.S = S_.ptr;
  d.rhs = rhs_.ptr;
  d.xchg_upd = xchg_upd_.ptr;
  d.xchg_chol = xchg_chol_.ptr;
  d.xc = S_.ptr + (size_t)n_ * n_;
  d.work = work_.ptr;
  d.stamps = stamp_on_ ? stamps_.ptr : nullptr;
  d.wt = wt_stores_;
  d.fd_pair = fd_pair_.ptr;
  d.obs_pnt = obs_pnt_.ptr;
  d.lchunks = lchunks_d_.ptr;
  d.lrounds = lrounds_d_.ptr;
  d.nlin = wk_.nlin;
  d.npu = wk_.npu;
  d.pu_units = pu_units_.ptr;
  d.segs = segs_.ptr;
  d.nseg = wk_.nseg;
  d.sbatch = sbatch_.ptr;
  d.pinfo = reinterpret_cast<const int2*>(pinfo_.ptr);
  d.pmx = reinterpret_cast<const int4*>(pmx_.ptr);
  d.cells = reinterpret_cast<const int4*>(cells_.ptr);
  d.cell_obs = cell_obs_.ptr;
  d.wsegs = wsegs_.ptr;
  d.nwide = wk_.nwide;
  d.stile = stile_.ptr;
  d.nstile = env_.nstile;
  d.stile_dst = stile_dst_.ptr;
  // St follows the separator terms in Wg_ (PlanChol: wg_size)
  const size_t npan = (size_t)(n_ + kCholNb - 1) / kCholNb;
  d.St = chol_.wg_size ? Wg_.ptr + 2 * npan * kTB * 256 + 16 * npan + 49 * 256 + 7 * 16 : nullptr;
  d.seg_fail = seg_fail_.ptr;
  d.pairs = reinterpret_cast<const int2*>(pairs_.ptr);
  d.assemble = (!comm_ || comm_->rank() == 0) ? 1 : 0;
  return d;
}

// The LM state handed over as a kernel argument (no host buffer, no copy engine: see hostmirror.h).
__global__ void k_set_state(LmState s, LmState* st) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *st = s;
}

// The current parameter slot's poses, points and intrinsics into the mapped download buffer
// [q 4F | t 3F | X 4P | k 7 ncam] (the slot is read on the device: no state round trip first).
__global__ __launch_bounds__(256) void k_download(const double* __restrict__ q, const double* __restrict__ t,
                                                  const double* __restrict__ X, const double* __restrict__ k,
                                                  const LmState* st, int F, int P, int ncam, double* __restrict__ out) {
  const int cur = st->cur;
  const size_t nq = 4 * (size_t)F, nt = 3 * (size_t)F, nx = 4 * (size_t)P, nk = 7 * (size_t)ncam;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nq + nt + nx + nk;
       i += (size_t)gridDim.x * blockDim.x) {
    double v;
    if (i < nq) v = q[nq * cur + i];
    else if (i < nq + nt) v = t[nt * cur + (i - nq)];
    else if (i < nq + nt + nx) v = X[nx * cur + (i - nq - nt)];
    else v = k[nk * cur + (i - nq - nt - nx)];
    out[i] = v;
  }
}

// Wait for stream s by spinning on an event query.  hipStreamSynchronize's blocking wait returned 13-28 ms
// late in a few percent of the main.cpp replay's loads, all of whose work had been three small kernels
// (tools/e2e_replay.py, profiles/r3_v8_*); the solver's waits are short (a load, an LM batch), so the host
// spins on them, falling back to the blocking wait after 200 ms.  A sharded solver (several
// ranks, possibly rank threads or processes sharing the host's cores with the threads that run the host
// all-reduces) yields between polls and spins at most 1 ms.
void BaSolver::WaitStream(hipStream_t s) {
  constexpr double spin_ms = 200.0;
  const bool shared = nranks() > 1;
  const double limit = shared ? std::min(spin_ms, 1.0) : spin_ms;
  if (!ev_wait_) SG_HIP_CHECK(hipEventCreateWithFlags(&ev_wait_, hipEventDisableTiming));
  SG_HIP_CHECK(hipEventRecord(ev_wait_, s));
  const auto t0 = std::chrono::steady_clock::now();
  while (true) {
    const hipError_t e = hipEventQuery(ev_wait_);
    if (e == hipSuccess) {
      MarkIdle(s);
      return;
    }
    if (e != hipErrorNotReady) SG_HIP_CHECK(e);
    if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > limit) break;
    if (shared) std::this_thread::yield();
  }
  SG_HIP_CHECK(hipEventSynchronize(ev_wait_));
  MarkIdle(s);
}

// SG_HOST_TIMING: a device marker and the host clock at the moment the stream was last seen idle, so a load can
// compare the device's and the host's time from there to its first command (a late queue start shows as a
// device gap longer than the host's).
void BaSolver::MarkIdle(hipStream_t s) {
  static const bool host_timing = getenv("SG_HOST_TIMING") != nullptr;
  if (!host_timing) return;
  if (!ev_idle_) SG_HIP_CHECK(hipEventCreate(&ev_idle_));
  SG_HIP_CHECK(hipEventRecord(ev_idle_, s));
  idle_host_ = std::chrono::steady_clock::now();
  idle_valid_ = true;
}

void BaSolver::DevMark(hipStream_t s, int i) {
  if (!dev_marks_[i]) SG_HIP_CHECK(hipEventCreate(&dev_marks_[i]));
  SG_HIP_CHECK(hipEventRecord(dev_marks_[i], s));
}

void BaSolver::ReadState(LmState* h) {
  static_assert(sizeof(LmState) % 8 == 0, "LmState is copied in 8-byte words");
  mb_.Reserve(1024);
  hipLaunchKernelGGL(k_copy_u64, dim3(1), dim3(64), 0, stream_, reinterpret_cast<const unsigned long long*>(st_.ptr),
                     reinterpret_cast<unsigned long long*>(mb_.d), sizeof(LmState) / 8);
  WaitStream(stream_);
  std::memcpy(h, mb_.h, sizeof(LmState));
}

void BaSolver::Begin(const sg_solver_options& o) {
  SG_REQUIRE(loaded_, SG_EINVAL, "no problem loaded");
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  const bool began_again = began_;
  if (began_) {
    // restart from the current parameter slot: move it to slot 0 (a fresh load starts in slot 0: no round trip)
    LmState h{};
    ReadState(&h);
    if (h.cur == 1) {
      SG_HIP_CHECK(hipMemcpyAsync(q_.ptr, q_.ptr + 4 * (size_t)F_, 4 * (size_t)F_ * 8, hipMemcpyDeviceToDevice, stream_));
      SG_HIP_CHECK(hipMemcpyAsync(t_.ptr, t_.ptr + 3 * (size_t)F_, 3 * (size_t)F_ * 8, hipMemcpyDeviceToDevice, stream_));
      SG_HIP_CHECK(hipMemcpyAsync(X_.ptr, X_.ptr + 4 * (size_t)P_, 4 * (size_t)P_ * 8, hipMemcpyDeviceToDevice, stream_));
      if (ncam_ > 0)
        SG_HIP_CHECK(hipMemcpyAsync(k_.ptr, k_.ptr + 7 * (size_t)ncam_, 7 * (size_t)ncam_ * 8, hipMemcpyDeviceToDevice,
                                    stream_));
    }
  }
  began_ = true;
  LmState s{};
  s.max_iter = o.max_num_iterations;
  s.max_invalid = o.max_num_consecutive_invalid_steps;
  s.disable_term = o.disable_termination;
  s.always_lin = o.always_linearize;
  s.jacobi = o.jacobi_scaling;
  s.ftol = o.function_tolerance;
  s.gtol = o.gradient_tolerance;
  s.ptol = o.parameter_tolerance;
  s.min_rel_dec = o.min_relative_decrease;
  s.max_radius = o.max_trust_region_radius;
  s.min_radius = o.min_trust_region_radius;
  s.min_diag = o.min_lm_diagonal;
  s.max_diag = o.max_lm_diagonal;
  s.cur = 0;
  s.need_lin = 1;
  s.first = 1;
  s.done = (NB_ == 0 && P_ == 0) ? 1 : 0;
  s.ok = 1;
  s.termination = s.done ? SG_FUNCTION_TOLERANCE : SG_NO_CONVERGENCE;
  s.radius = o.initial_trust_region_radius;
  s.decrease_factor = 2.0;
  hipLaunchKernelGGL(k_set_state, dim3(1), dim3(64), 0, stream_, s, st_.ptr);
  if (began_again && knobs_.spec) {
    // k_cam_reduce keeps the wide-chunk camera accumulators in speculative mode: clear both slots for the
    // restart's first k_linearize (a fresh Load has zeroed them)
    ZeroList z{};
    z.p[0] = cam_wide_.ptr;
    z.n[0] = cam_wide_.size;
    hipLaunchKernelGGL(k_reset_buffers, dim3(1), dim3(256), 0, stream_, z);
  }
  need_seq_ = true;   // the first iteration fixes the camera scale: k_schur waits for it
  pending_decision_ = false;
  for (auto& t : timers_) {
    t.total_ms = 0.0;
    t.count = 0;
  }
}

void BaSolver::TimedLaunchBegin(int id) { TimedLaunchBegin(id, stream_); }
void BaSolver::TimedLaunchEnd(int id) { TimedLaunchEnd(id, stream_); }
void BaSolver::TimedLaunchBegin(int id, hipStream_t s) {
  if (!timing_) return;
  hipEvent_t a, b;
  SG_HIP_CHECK(hipEventCreate(&a));
  SG_HIP_CHECK(hipEventCreate(&b));
  timers_[id].ev.push_back(a);
  timers_[id].ev.push_back(b);
  SG_HIP_CHECK(hipEventRecord(a, s));
}
void BaSolver::TimedLaunchEnd(int id, hipStream_t s) {
  if (!timing_) return;
  SG_HIP_CHECK(hipEventRecord(timers_[id].ev.back(), s));
}

void BaSolver::Iterate(int n) {
  SG_REQUIRE(loaded_, SG_EINVAL, "no problem loaded");
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  EnqueueIterations(n);
}

// The timer an op's launches are counted under (-1: none), in ChainOp's order.
static const int kChainTimer[(int)ChainOp::kCount] = {
    kKLin,        // Linearize
    kKCamReduce,  // CamReduce (the closing one, with two extra workgroups, counts as the update reduce: below)
    kKDecide,     // Decide
    -1,           // AllReduceCam
    -1,           // IntrLinearize
    kKCamFinal,   // CamFinalize
    kKSchur,      // Schur
    kKSReduce,    // SReduce
    -1,           // IntrSchur
    kKXchg,       // Exchange: pack, all-reduce, unpack
    kKChol,       // Chol
    -1,           // IntrStep
    kKPointUpd,   // UpdateLin
    kKPointUpd,   // PointUpdate
    kKUpdRed,     // UpdReduce
    -1,           // AllReduceUpd
};

// Enqueue n LM iterations: the launches ba_chain.cpp plans for each (which, in which order and mode: see there), with
// the grids, buffers and the Cholesky kernel the load chose.
void BaSolver::EnqueueIterations(int n) {
  const Dev d = MakeDev();
  const ChainShape shape{comm_ && comm_->nranks() > 1, d.assemble != 0, nk_, chol_.tiles, chol_.border};
  const int nv = NB_ * kCamV;
  const int npanel = (n_ + kCholNb - 1) / kCholNb;
  const dim3 pg(npanel + 1, 4);   // k_S_pack / k_S_unpack_fin
  const int32_t* panel_jend = (const int32_t*)work_i_.ptr;
  const int32_t* pack_off = (const int32_t*)pack_off_.ptr;
  auto run = [&](const ChainStep& step) {
    for (int i = 0; i < step.n; ++i) {
      const ChainCall c = step.ops[i];
      const int timer = c.op == ChainOp::CamReduce && c.a == 2 ? (int)kKUpdRed : kChainTimer[(int)c.op];
      if (timer >= 0) TimedLaunchBegin(timer);
      switch (c.op) {
        case ChainOp::Linearize: LaunchLinearize(d); break;
        case ChainOp::CamReduce: LaunchCamReduceK(NB_ + c.a, stream_, d, c.b); break;
        case ChainOp::Decide: LaunchDecideK(stream_, d, c.a); break;
        case ChainOp::AllReduceCam: AllReduceSum(xchg_cam_.ptr, (size_t)nv + kXNum + nranks()); break;
        case ChainOp::IntrLinearize: LaunchIntrLinearizeK(stream_, d, n_, nk_, NB_, ncam_, M_, wk_.intr_nsl); break;
        case ChainOp::CamFinalize: LaunchCamFinalizeK(stream_, d, c.a, 0); break;
        case ChainOp::Schur: LaunchSchurK(std::max(wk_.nseg, 1), wk_.nwide, c.a, stream_, d); break;
        case ChainOp::SReduce: LaunchSReduceK(std::max(env_.nstile + NB_, 1), stream_, d, c.a, c.b); break;
        case ChainOp::IntrSchur: LaunchIntrSchurK(stream_, d, n_, nk_, NB_, ncam_, P_, wk_.intr_nsl); break;
        case ChainOp::Exchange:
          LaunchSPackK(pg, stream_, S_.ptr, n_, panel_jend, pack_off, npanel, Spk_.ptr, 0);
          AllReduceSum(Spk_.ptr, env_.npack + (c.a ? ntail_ : 0));
          if (c.b)
            LaunchSUnpackFinK(pg, stream_, d, panel_jend, pack_off, npanel, Spk_.ptr);
          else
            LaunchSPackK(pg, stream_, S_.ptr, n_, panel_jend, pack_off, npanel, Spk_.ptr, 1);
          break;
        case ChainOp::Chol:
          if (chol_.tiles)
            LaunchCholTiles(d.stamps != nullptr, dim3(chol_.nd > 0 ? 2 : 1), d,
                            (chol_.cand_lds ? 2 : 0) | (knobs_.chol_force_tmo ? 4 : 0) | (c.a ? 16 : 0) | (c.b ? 32 : 0) |
                                knobs_.chol_delay);
          else if (chol_.window)
            LaunchCholWindowK(d.stamps != nullptr, stream_, d, panel_jend, rdg_.ptr);
          else
            LaunchCholGlobalK(chol_.gstage, (size_t)std::max(n_, 1) * 8 * (chol_.gstage ? 1 + kCholNb : 1), stream_, d,
                              panel_jend, rdg_.ptr);
          break;
        case ChainOp::IntrStep: LaunchIntrStepK(stream_, d); break;
        case ChainOp::UpdateLin: LaunchUpdateLin(d); break;
        case ChainOp::PointUpdate: LaunchPointUpdateK(std::max(wk_.npu, 1), stream_, d); break;
        case ChainOp::UpdReduce: LaunchUpdReduceK(stream_, d, c.a); break;
        case ChainOp::AllReduceUpd: AllReduceSum(xchg_upd_.ptr, kUNum); break;
        case ChainOp::kCount: break;
      }
      if (timer >= 0) TimedLaunchEnd(timer);
    }
  };
  for (int it = 0; it < n; ++it) {
    const ChainStep step = PlanIteration(shape, knobs_, need_seq_, pending_decision_);
    run(step);
    need_seq_ = false;
    pending_decision_ = step.pending_out;
    chol_stile_last_ = step.stile;
  }
  run(PlanBatchTail(pending_decision_));
  pending_decision_ = false;
  SG_HIP_CHECK(hipGetLastError());
}

__global__ void k_force_linearize(LmState* st) {
  if (threadIdx.x == 0) {
    st->need_lin = 1;
    st->done = 0;
  }
}

void BaSolver::Sweep(int n) {
  SG_REQUIRE(loaded_, SG_EINVAL, "no problem loaded");
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  Dev d = MakeDev();
  for (int it = 0; it < n; ++it) {
    hipLaunchKernelGGL(k_force_linearize, dim3(1), dim3(64), 0, stream_, st_.ptr);
    TimedLaunchBegin(kKLin);
    LaunchLinearize(d);
    TimedLaunchEnd(kKLin);
  }
  SG_HIP_CHECK(hipGetLastError());
}

void BaSolver::LaunchLinearize(const Dev& d) { LaunchLinearizeK(wk_.lin_waves, std::max(wk_.nlin, 1), stream_, d); }

void BaSolver::LaunchUpdateLin(const Dev& d) {
  LaunchUpdateLinK(stamp_on_, wk_.lin_waves, std::max(wk_.nlin, 1), stream_, d);
}

std::vector<unsigned long long> BaSolver::Stamps() {
  std::vector<unsigned long long> v(stamp_on_ ? stamps_.size : 64, 0);
  if (!stamp_on_) return v;
  SG_HIP_CHECK(hipMemcpyAsync(v.data(), stamps_.ptr, v.size() * 8, hipMemcpyDeviceToHost, stream_));
  SG_HIP_CHECK(hipStreamSynchronize(stream_));
  return v;
}

void BaSolver::Sync() { SG_HIP_CHECK(hipStreamSynchronize(stream_)); }

void BaSolver::Summary(sg_solver_summary* s) {
  LmState h{};
  ReadState(&h);
  std::memset(s, 0, sizeof(*s));
  s->num_iterations = h.pushed;
  s->num_successful_steps = h.n_succ;
  s->num_unsuccessful_steps = h.n_unsucc;
  s->num_invalid_steps = h.n_invalid;
  s->termination_type = h.termination;
  s->ok = h.ok;
  s->initial_cost = h.initial_cost;
  s->final_cost = h.min_pushed_cost + h.fixed_cost;
  s->fixed_cost = h.fixed_cost;
  s->trust_region_radius = h.radius;
  s->num_lm_iterations = h.lm_iters;
  s->sync_timeouts = h.sync_timeouts;
}

void BaSolver::Download(sg_problem* p) {
  const size_t nq = 4 * (size_t)F_, nt = 3 * (size_t)F_, nx = 4 * (size_t)P_, nk = nk_ ? 7 * (size_t)ncam_ : 0;
  const size_t tot = nq + nt + nx + nk;
  mb_.Reserve(1024 + 8 * std::max<size_t>(tot, 1));
  double* out_d = reinterpret_cast<double*>(mb_.d + 1024);
  const double* out = reinterpret_cast<const double*>(mb_.h + 1024);
  const unsigned g = (unsigned)std::min<size_t>(1024, std::max<size_t>(1, (tot + 255) / 256));
  hipLaunchKernelGGL(k_download, dim3(g), dim3(256), 0, stream_, q_.ptr, t_.ptr, X_.ptr, nk ? k_.ptr : q_.ptr,
                     (const LmState*)st_.ptr, F_, P_, nk ? ncam_ : 0, out_d);
  WaitStream(stream_);
  std::copy(out, out + nq, p->q);
  std::copy(out + nq, out + nq + nt, p->t);
  const double* X = out + nq + nt;
  for (int i = 0; i < P_; ++i) {
    const int pt = point_perm_[i];
    for (int a = 0; a < 4; ++a) p->X[4 * pt + a] = X[4 * i + a];
  }
  if (nk) std::copy(out + nq + nt + nx, out + tot, p->k);
}

void BaSolver::Solve(const sg_solver_options& o, sg_problem* p, sg_solver_summary* s) {
  Begin(o);
  const int batch = 8;
  LmState h{};
  const long long cap = (long long)o.max_num_iterations * (o.max_num_consecutive_invalid_steps + 2) + 16;
  long long launched = 0;
  while (true) {
    Iterate(batch);
    launched += batch;
    ReadState(&h);
    if (h.done) break;
    SG_REQUIRE(launched < cap, SG_EDEVICE, "LM loop did not terminate on the device");
  }
  Summary(s);
  Download(p);
}

void BaSolver::Evaluate(double* residuals, double* cost, int32_t* nfail) {
  SG_REQUIRE(loaded_, SG_EINVAL, "no problem loaded");
  DBuf<double> r, c;
  DBuf<int32_t> nf;
  r.Resize(2 * (size_t)std::max(M_, 1));
  c.Resize(1);
  nf.Resize(1);
  c.Zero(stream_);
  nf.Zero(stream_);
  Dev d = MakeDev();
  if (M_ > 0)
    LaunchEvaluateK(M_, stream_, d, r.ptr, c.ptr, nf.ptr);
  std::vector<double> rh(2 * (size_t)M_);
  if (M_ > 0) SG_HIP_CHECK(hipMemcpyAsync(rh.data(), r.ptr, rh.size() * 8, hipMemcpyDeviceToHost, stream_));
  SG_HIP_CHECK(hipMemcpyAsync(cost, c.ptr, 8, hipMemcpyDeviceToHost, stream_));
  SG_HIP_CHECK(hipMemcpyAsync(nfail, nf.ptr, 4, hipMemcpyDeviceToHost, stream_));
  SG_HIP_CHECK(hipStreamSynchronize(stream_));
  for (int o = 0; o < M_; ++o) {
    residuals[2 * obs_perm_[o]] = rh[2 * o];
    residuals[2 * obs_perm_[o] + 1] = rh[2 * o + 1];
  }
}

void BaSolver::SetTiming(bool on) {
  timing_ = on;
  for (auto& t : timers_) {
    for (auto e : t.ev) (void)hipEventDestroy(e);
    t.ev.clear();
    t.total_ms = 0.0;
    t.count = 0;
  }
}

void BaSolver::CollectTimes() {
  SG_HIP_CHECK(hipStreamSynchronize(stream_));
  for (auto& t : timers_) {
    for (size_t i = 0; i + 1 < t.ev.size(); i += 2) {
      float ms = 0.f;
      SG_HIP_CHECK(hipEventElapsedTime(&ms, t.ev[i], t.ev[i + 1]));
      t.total_ms += ms;
      t.count += 1;
    }
    for (auto e : t.ev) (void)hipEventDestroy(e);
    t.ev.clear();
  }
}

int BaSolver::KernelTimes(char* names, int names_len, double* ms, int32_t* counts, int max) {
  CollectTimes();
  std::string all;
  int k = 0;
  for (auto& t : timers_) {
    if (k < max) {
      ms[k] = t.count ? t.total_ms / t.count : 0.0;
      counts[k] = t.count;
    }
    if (!all.empty()) all += ",";
    all += t.name;
    ++k;
  }
  if (names && names_len > 0) {
    std::strncpy(names, all.c_str(), names_len - 1);
    names[names_len - 1] = 0;
  }
  return std::min(k, max);
}

// Algorithmic bytes / flops per launch (for the roofline line in bench.py).
int BaSolver::KernelWork(double* bytes, double* flops, int max) {
  const double M = M_, P = P_, n = n_, NB = NB_;
  double npairs = 0.0;  // observation pairs of free points on free frames are not tracked here: use M*k/2
  (void)npairs;
  std::vector<double> by(kKNum, 0.0), fl(kKNum, 0.0);
  // linearize: read obs (16 B pt + 4 B frame + 1 B fixed) + point X 32 B + offsets 4 B; write the J record
  // (kJStride doubles: 128 B since round 6), V 80 B, g 32 B per point; camera partials
  const double jrec = 8.0 * kJStride;
  by[kKLin] = M * (16 + 4 + 1 + jrec) + P * (32 + 4 + 80 + 32 + 1) + NB * kCamV * 8;
  fl[kKLin] = M * 420.0;
  // k_schur: the record less r~ (rotation pairs + J~p) and the observation meta; per point V, g, scales, X.w and
  // the written Vinv / t / diag
  by[kKSchur] = M * (jrec - 16 + 4) + P * (80 + 32 + 32 + 8 + 32 + 80 + 32);
  fl[kKSchur] = 2048.0 * wk_.schur_mfma + 512.0 * wk_.schur_rhs;   // 16x16x4 tile updates, 4x4x4 (4-block) rhs slots
  by[kKPointUpd] = M * (jrec + 16 + 4) + P * (32 + 32 + 80 + 32 + 32);
  if (knobs_.spec) {   // k_update_lin: the update's traffic plus the candidate's linearization (a second J record, V, g)
    by[kKPointUpd] = M * (jrec + jrec + 16 + 4 + 4 + 4) + P * (32 + 32 + 80 + 32 + 32 + 80 + 32) + NB * kCamV * 8;
    fl[kKPointUpd] = M * 420.0;
  }
  by[kKChol] = n * n * 8 * 2;
  fl[kKChol] = n * n * n / 3.0;
  int k = 0;
  for (; k < std::min(max, (int)kKNum); ++k) {
    bytes[k] = by[k];
    flops[k] = fl[k];
  }
  // derived figures after the kernels (bench.py's roofline fields):
  //   [kKNum]     k_schur's useful flops: the MFMA slots of each point's own tiles (its first to its last window
  //               tile), without the slots that multiply the zero tiles left of its first column
  //   [kKNum + 1] SURVEY 8d's algorithmic bytes of one linearization sweep at the reference's f64: per observation
  //               uv 16 + frame index 4 + r 16 + W_ip 192, per point CSR offset 4 + X 32 + V_p 80 + g_p 32, per
  //               camera block pose 56 + U_i / g_c 8 (21 + 6)
  if (max > kKNum) {
    bytes[kKNum] = 0.0;
    flops[kKNum] = wk_.schur_useful;
    ++k;
  }
  if (max > kKNum + 1) {
    bytes[kKNum + 1] = M * 228.0 + P * 148.0 + NB * (56.0 + 8.0 * 27);
    flops[kKNum + 1] = 0.0;
    ++k;
  }
  return k;
}

void BaSolver::Info(sg_ba_info* o) const {
  std::memset(o, 0, sizeof(*o));
  o->num_frames = F_;
  o->num_points = P_;
  o->num_obs = M_;
  o->num_blocks = NB_;
  o->n = n_;
  o->band_tiles = env_.band_tiles;
  o->cholesky_path = chol_.border ? 4 : chol_.tiles ? 0 : (chol_.window ? 1 : (chol_.gstage ? 2 : 3));
  o->cholesky_split = chol_.tiles ? chol_.nd : 0;
  o->num_pairs = (int32_t)std::min<size_t>(wk_.npairs, INT32_MAX);
  o->rank = comm_ ? comm_->rank() : 0;
  o->nranks = comm_ ? comm_->nranks() : 1;
  o->num_allreduces = nallreduce_;
  o->lin_waves = wk_.lin_waves;
  o->cholesky_separator = chol_.tiles && chol_.nd > 0 ? chol_.ns : 0;
  o->cholesky_stile = chol_stile_last_ ? 1 : 0;
  o->wt_stores = wt_stores_;
}

double BaSolver::ReprojectMap(sg_map* m) {
  SG_HIP_CHECK(hipSetDevice(dev_.device));
  const int M = m->num_obs;
  hipStream_t s = stream_;
  io_.Begin();
  io_.Up(mk_, m->k, 7 * (size_t)m->num_cameras);
  io_.Up(mq_, m->q, 4 * (size_t)m->num_frames);
  io_.Up(mt_, m->t, 3 * (size_t)m->num_frames);
  io_.Up(mX_, m->X, 4 * (size_t)m->num_points);
  io_.Up(mobs_pt_, m->obs_pt, 2 * (size_t)M);
  io_.Up(mobs_frame_, m->obs_frame, (size_t)M);
  io_.Up(mobs_point_, m->obs_point, (size_t)M);
  io_.Up(mframe_cam_, m->frame_camera, (size_t)m->num_frames);
  io_.FlushUp(s);
  mobs_err_.Resize(2 * (size_t)std::max(M, 1));
  const int nb = std::max((M + 255) / 256, 1);
  mred_.Resize(2 * (size_t)nb + 2);   // (every block writes its partial: no zeroing)
  LaunchReprojectMapK(M, nb, s, mk_.ptr, mq_.ptr, mt_.ptr, mframe_cam_.ptr, mX_.ptr, mobs_pt_.ptr, mobs_frame_.ptr,
                      mobs_point_.ptr, mobs_err_.ptr, mred_.ptr);
  SG_HIP_CHECK(hipGetLastError());
  double out[2] = {0, 0};
  io_.Down(m->obs_error, mobs_err_.ptr, 2 * (size_t)M * 8);
  io_.Down(out, mred_.ptr + 2 * nb, 16);
  io_.FinishDown(s);
  return out[0];
}

}  // namespace sg
