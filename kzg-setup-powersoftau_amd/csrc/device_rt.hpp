// Device-side helpers of the C ABI units (capi.hip, preprocess.hip, phase2.hip): HIP error
// handling, the bad-key protocol of every launch, the current device and per-call device memory.
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

}  // namespace kzgpot
