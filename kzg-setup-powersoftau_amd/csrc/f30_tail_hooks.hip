// Test build only (libkzgpot_test.so, -DKZGPOT_TEST_HOOKS; tests/kzgpot_test_f30_tail_hooks.h): one tail
// form of the radix-2^30 scans (fp381.hpp f30_mul<K0, K1> / f30_sqr<K0, K1>) per lane on caller-supplied
// digit arrays, so that tests/test_gpu_f30_tail.py can compare the output DIGITS with the exact model
// tests/f30_tail_model.py, with tail digits, column sums, carries and the top digit at their bounds.
#ifdef KZGPOT_TEST_HOOKS
#include "../../tests/kzgpot_test_f30_tail_hooks.h"
#include "device_rt.hpp"
#include "fp381.hpp"

using namespace kzgpot;

namespace {

constexpr int kBlock = 256;

// operands and results are lane-major: 13 int32 digits per lane, lane i at [13 i, 13 i + 13)
__device__ __forceinline__ void f30_load(f30& x, const int32_t* p, long i) {
#pragma unroll
  for (int k = 0; k < N30; k++) x.v[k] = p[N30 * i + k];
}

constexpr bool is_mul(int op) { return op == KZGPOT_F30_TAIL_MUL_M1 || op == KZGPOT_F30_TAIL_MUL_M16_64; }
constexpr int tails(int op) { return op == KZGPOT_F30_TAIL_MUL_M1 || op == KZGPOT_F30_TAIL_SQR_M2 ? 1 : 2; }

template <int OP>
__global__ void __launch_bounds__(kBlock) k_f30_tail_op(long n, const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                        const int32_t* __restrict__ t0, const int32_t* __restrict__ t1,
                                                        int32_t* __restrict__ r) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  f30 x, y, u, v, o;
  f30_load(x, a, i);
  if (is_mul(OP)) f30_load(y, b, i);
  f30_load(u, t0, i);
  if (tails(OP) == 2) f30_load(v, t1, i);
  if (OP == KZGPOT_F30_TAIL_MUL_M1) f30_mul<-1>(o, x, y, u);
  if (OP == KZGPOT_F30_TAIL_SQR_M2) f30_sqr<-2>(o, x, u);
  if (OP == KZGPOT_F30_TAIL_SQR_M1_M2) f30_sqr<-1, -2>(o, x, u, v);
  if (OP == KZGPOT_F30_TAIL_SQR_M1_M1) f30_sqr<-1, -1>(o, x, u, v);
  if (OP == KZGPOT_F30_TAIL_MUL_M16_64) f30_mul<-16, 64>(o, x, y, u, v);
#pragma unroll
  for (int k = 0; k < N30; k++) r[N30 * i + k] = o.v[k];
}

template <int OP>
int run_op(long n, const int32_t* a, const int32_t* b, const int32_t* t0, const int32_t* t1, int32_t* r) {
  const int32_t* in[4] = {a, b, t0, t1};
  const bool used[4] = {true, is_mul(OP), true, tails(OP) == 2};
  for (int k = 0; k < 4; k++)
    if (used[k] && !in[k]) return KZGPOT_E_INVALID_ARG;
  if (device_count() <= 0) return KZGPOT_E_DEVICE;
  const size_t bytes = (size_t)n * N30 * sizeof(int32_t);
  DevBuf din[4], dout;
  for (int k = 0; k < 4; k++) {
    if (!used[k]) continue;
    if (din[k].alloc(bytes)) return KZGPOT_E_DEVICE;
    HIP_TRY(hipMemcpy(din[k].p, in[k], bytes, hipMemcpyHostToDevice));
  }
  if (dout.alloc(bytes)) return KZGPOT_E_DEVICE;
  const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_f30_tail_op<OP>, dim3(blocks), dim3(kBlock), 0, nullptr, n, (const int32_t*)din[0].p,
                     (const int32_t*)din[1].p, (const int32_t*)din[2].p, (const int32_t*)din[3].p, (int32_t*)dout.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(r, dout.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" int kzgpot_test_f30_tail_op(int op, long n, const int32_t* a, const int32_t* b, const int32_t* t0,
                                       const int32_t* t1, int32_t* r) {
  if (n <= 0 || n > (1 << 20) || !r) return KZGPOT_E_INVALID_ARG;
  switch (op) {
    case KZGPOT_F30_TAIL_MUL_M1: return run_op<KZGPOT_F30_TAIL_MUL_M1>(n, a, b, t0, t1, r);
    case KZGPOT_F30_TAIL_SQR_M2: return run_op<KZGPOT_F30_TAIL_SQR_M2>(n, a, b, t0, t1, r);
    case KZGPOT_F30_TAIL_SQR_M1_M2: return run_op<KZGPOT_F30_TAIL_SQR_M1_M2>(n, a, b, t0, t1, r);
    case KZGPOT_F30_TAIL_SQR_M1_M1: return run_op<KZGPOT_F30_TAIL_SQR_M1_M1>(n, a, b, t0, t1, r);
    case KZGPOT_F30_TAIL_MUL_M16_64: return run_op<KZGPOT_F30_TAIL_MUL_M16_64>(n, a, b, t0, t1, r);
    default: return KZGPOT_E_INVALID_ARG;
  }
}
#endif  // KZGPOT_TEST_HOOKS
