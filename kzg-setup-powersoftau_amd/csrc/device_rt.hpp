// Device-side helpers of the C ABI units (capi.hip, preprocess.hip, phase2.hip, msm.hip, open.hip,
// domain.hip, evals.hip, pairing.hip, verify.hip) and of the test hooks: HIP error handling, the
// bad-key protocol of every launch, the current device, per-call device memory and the host-buffer
// form of a `_dev` entry point (StagedCall).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/kzgpot.h"

namespace kzgpot {

constexpr uint64_t kNoBad = ~0ull;

#define HIP_TRY(expr)                                                                    \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      fprintf(stderr, "kzgpot: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), \
              __FILE__, __LINE__);                                                       \
      return KZGPOT_E_DEVICE;                                                            \
    }                                                                                    \
  } while (0)

inline int decode_key(uint64_t key, int64_t* first_bad) {
  // no kernel writes key 0 (every rejection has status >= 1): it is the multi-rank "a rank failed"
  // word (KZGPOT_KEY_RANK_FAILED), never "point 0 accepted"
  if (key == kNoBad || key == KZGPOT_KEY_RANK_FAILED) {
    if (first_bad) *first_bad = -1;
    return key == kNoBad ? 0 : KZGPOT_E_RANK_FAILED;
  }
  if (first_bad) *first_bad = (int64_t)(key >> 8);
  return -(int)(key & 0xff);
}

// The bad-key protocol of a launch: the key is set to all-ones (kNoBad) on `stream`, then `launch`
// enqueues kernels there that lower it to (index << 8 | status) of their first rejected point.
// host_key (optional) receives it once those kernels are done.
template <class Launch>
int launch_with_key(uint64_t* d_key, hipStream_t stream, Launch&& launch, uint64_t* host_key = nullptr) {
  HIP_TRY(hipMemsetAsync(d_key, 0xff, sizeof(uint64_t), stream));
  HIP_TRY(launch((unsigned long long*)d_key));
  if (host_key) {
    *host_key = kNoBad;
    HIP_TRY(hipMemcpyAsync(host_key, d_key, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
  }
  return 0;
}

inline int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

inline int current_device() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) return -1;
  return d;
}

// Restores the caller's current HIP device on scope exit: the library switches devices per
// shard, and a torch rank on cuda:3 must still be on cuda:3 after any call.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// device memory of one call, freed on every exit path (hipFree waits for the work that uses it)
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t n) {
    HIP_TRY(hipMalloc(&p, n ? n : 1));
    return 0;
  }
};

// The host-buffer form of a `_dev` entry point: the same call on the caller's host memory, synchronous,
// on the null stream of the current device. Its contract, for every entry point that has one:
//   - the function resets *first_bad and checks its arguments (KZGPOT_E_INVALID_ARG) before it declares a
//     StagedCall, so an argument error uses no device;
//   - begin() is the first step: KZGPOT_E_DEVICE without a device, before anything is allocated or written;
//   - inputs go through per-call device buffers, all freed on every exit path; any HIP failure is
//     KZGPOT_E_DEVICE;
//   - finish() takes the `_dev` call's return value. A keyed call's key is read there: a rejection returns
//     decode_key() and NOTHING is written to a caller buffer; otherwise `out` copies the results out;
//   - the caller's current device is restored on return.
// Every step but finish() returns 0 or KZGPOT_E_DEVICE, so the steps chain with ||.
class StagedCall {
 public:
  uint64_t* d_key = nullptr;  // the key word of a keyed call, once key() has run

  int begin() { return device_count() > 0 ? 0 : KZGPOT_E_DEVICE; }
  // d = `bytes` of device memory (0: a valid 1-byte buffer)
  template <class T>
  int alloc(T*& d, size_t bytes) {
    if (used_ == kMaxBufs || bufs_[used_].alloc(bytes)) return KZGPOT_E_DEVICE;
    d = (T*)bufs_[used_++].p;
    return 0;
  }
  // `bytes` of host memory to d, which may point into a buffer of alloc()'s (0: src is not read)
  int copy_in(void* d, const void* src, size_t bytes) {
    if (bytes) HIP_TRY(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    return 0;
  }
  template <class T>
  int in(T*& d, const void* src, size_t bytes) {
    return alloc(d, bytes) || copy_in(d, src, bytes) ? KZGPOT_E_DEVICE : 0;
  }
  int key() { return alloc(d_key, sizeof(uint64_t)); }
  // rc: what the `_dev` call on the null stream returned; first_bad: null for a call without a key
  template <class Out>
  int finish(int rc, int64_t* first_bad, Out&& out) {
    if (rc) return rc;
    uint64_t k = kNoBad;
    if (d_key)
      HIP_TRY(hipMemcpy(&k, d_key, sizeof k, hipMemcpyDeviceToHost));
    else
      HIP_TRY(hipStreamSynchronize(nullptr));
    if (k != kNoBad) return decode_key(k, first_bad);  // rejected: nothing is written
    return out();
  }

 private:
  static constexpr int kMaxBufs = 8;
  DeviceGuard guard_;
  DevBuf bufs_[kMaxBufs];
  int used_ = 0;
};

inline int copy_out(void* dst, const void* d, size_t bytes) {
  HIP_TRY(hipMemcpy(dst, d, bytes, hipMemcpyDeviceToHost));
  return 0;
}

// The verdict of a pairing product's or a check's d_out (GT bytes, then the u32): 1 or 0
inline int read_verdict(const void* d_out) {
  uint32_t v;
  HIP_TRY(hipMemcpy(&v, (const uint8_t*)d_out + KZGPOT_GT_BYTES, sizeof v, hipMemcpyDeviceToHost));
  return v ? 1 : 0;
}

}  // namespace kzgpot
