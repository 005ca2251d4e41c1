// device_stream.h — the two value types the device-pass handles (PoseSolver, PointSolver, AlignSolver, RelPoseSolver,
// PoseGraphSolver, MatchSolver, EpipolarSolver, MapOps) hold as members: the stream a handle runs on, and the HIP-event
// timer behind its SetTiming / last_kernel_ms.  A handle declares its DeviceStream before its buffers and HostIo, so
// they are destroyed while the stream still exists.
#ifndef SG_DEVICE_STREAM_H_
#define SG_DEVICE_STREAM_H_

#include <hip/hip_runtime.h>

#include "common.h"

namespace sg {

// The device a handle runs on and its stream: the caller's (borrowed: the Slam facade passes its solver's), or one
// created here and destroyed with the handle.
class DeviceStream {
 public:
  explicit DeviceStream(const sg_device_options& dev, hipStream_t borrowed = nullptr)
      : device_(dev.device), stream_(borrowed) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) throw Error(SG_ENODEV, "no HIP device available");
    SG_REQUIRE(device_ >= 0 && device_ < ndev, SG_ENODEV, "device ordinal out of range");
    SG_HIP_CHECK(hipSetDevice(device_));
    if (!borrowed) {
      SG_HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
      owned_ = true;
    }
  }
  ~DeviceStream() {
    if (owned_) (void)hipStreamDestroy(stream_);
  }
  DeviceStream(const DeviceStream&) = delete;
  DeviceStream& operator=(const DeviceStream&) = delete;

  hipStream_t get() const { return stream_; }
  int device() const { return device_; }
  // Makes the handle's device the calling thread's: what every call that touches the device begins with.
  void Bind() const { SG_HIP_CHECK(hipSetDevice(device_)); }

 private:
  int device_;
  hipStream_t stream_;
  bool owned_ = false;
};

// HIP-event time of the launches between Start and Stop, when enabled.  A call begins with Reset; Read comes after the
// stream has been waited on (both events have completed).  A call that launches nothing therefore reports 0.0.
class KernelTimer {
 public:
  KernelTimer() = default;
  ~KernelTimer() {
    for (hipEvent_t e : ev_)
      if (e) (void)hipEventDestroy(e);
  }
  KernelTimer(const KernelTimer&) = delete;
  KernelTimer& operator=(const KernelTimer&) = delete;

  void Enable(bool on) { on_ = on; }
  void Reset() {
    started_ = false;
    ms_ = 0.0;
  }
  void Start(hipStream_t s) {
    started_ = false;
    if (!on_) return;
    for (hipEvent_t& e : ev_)
      if (!e) SG_HIP_CHECK(hipEventCreate(&e));
    SG_HIP_CHECK(hipEventRecord(ev_[0], s));
    started_ = true;
  }
  void Stop(hipStream_t s) {
    if (started_) SG_HIP_CHECK(hipEventRecord(ev_[1], s));
  }
  double Read() {
    ms_ = 0.0;
    if (started_) {
      float ms = 0.f;
      SG_HIP_CHECK(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
      ms_ = ms;
      started_ = false;
    }
    return ms_;
  }
  double last_ms() const { return ms_; }

 private:
  bool on_ = false, started_ = false;
  double ms_ = 0.0;
  hipEvent_t ev_[2] = {nullptr, nullptr};
};

}  // namespace sg

#endif  // SG_DEVICE_STREAM_H_
