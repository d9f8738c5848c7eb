// Test build only (libkzgpot_test.so, -DKZGPOT_TEST_HOOKS; tests/kzgpot_test_f30_hooks.h): one function of
// the radix-2^30 field core (fp381.hpp f30_*) per lane on caller-supplied digit arrays, so that
// tests/test_gpu_f30_core.py can compare the functions' output DIGITS with an exact integer model —
// the codec tests see only canonical bytes and cannot steer an internal digit to the edge of a bound.
#ifdef KZGPOT_TEST_HOOKS
#include "../../tests/kzgpot_test_f30_hooks.h"
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

constexpr int arity(int op) {
  return op == KZGPOT_F30_MUL_SUM2 ? 4
         : op == KZGPOT_F30_MUL_ADDSQR ? 3
         : op == KZGPOT_F30_MUL ? 2
                                : 1;
}

template <int OP>
__global__ void __launch_bounds__(kBlock) k_f30_op(long n, const int32_t* __restrict__ a, const int32_t* __restrict__ b,
                                                   const int32_t* __restrict__ c, const int32_t* __restrict__ d,
                                                   int32_t* __restrict__ r) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  f30 x, y, z, w, o;
  f30_load(x, a, i);
  if (arity(OP) >= 2) f30_load(y, b, i);
  if (arity(OP) >= 3) f30_load(z, c, i);
  if (arity(OP) >= 4) f30_load(w, d, i);
  if (OP == KZGPOT_F30_MUL) f30_mul(o, x, y);
  if (OP == KZGPOT_F30_SQR) f30_sqr(o, x);
  if (OP == KZGPOT_F30_MUL_ADDSQR) f30_mul_addsqr(o, x, y, z);
  if (OP == KZGPOT_F30_MUL_SUM2) f30_mul_sum2(o, x, y, z, w);
  if (OP == KZGPOT_F30_DBL) f30_dbl(o, x);
  if (OP == KZGPOT_F30_MUL3) f30_mul3(o, x);
  if (OP == KZGPOT_F30_NORM0) f30_norm<0>(o, x);
  if (OP == KZGPOT_F30_NORM1) f30_norm<1>(o, x);
  if (OP == KZGPOT_F30_NORM2) f30_norm<2>(o, x);
  if (OP == KZGPOT_F30_NORM3) f30_norm<3>(o, x);
#pragma unroll
  for (int k = 0; k < N30; k++) r[N30 * i + k] = o.v[k];
}

template <int OP>
int run_op(long n, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d, int32_t* r) {
  constexpr int n_in = arity(OP);
  const int32_t* in[4] = {a, b, c, d};
  for (int k = 0; k < n_in; k++)
    if (!in[k]) return KZGPOT_E_INVALID_ARG;
  if (device_count() <= 0) return KZGPOT_E_DEVICE;
  const size_t bytes = (size_t)n * N30 * sizeof(int32_t);
  DevBuf din[4], dout;
  for (int k = 0; k < n_in; k++) {
    if (din[k].alloc(bytes)) return KZGPOT_E_DEVICE;
    HIP_TRY(hipMemcpy(din[k].p, in[k], bytes, hipMemcpyHostToDevice));
  }
  if (dout.alloc(bytes)) return KZGPOT_E_DEVICE;
  const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_f30_op<OP>, dim3(blocks), dim3(kBlock), 0, nullptr, n, (const int32_t*)din[0].p,
                     (const int32_t*)din[1].p, (const int32_t*)din[2].p, (const int32_t*)din[3].p, (int32_t*)dout.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(r, dout.p, bytes, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" int kzgpot_test_f30_op(int op, long n, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d,
                                  int32_t* r) {
  if (n <= 0 || n > (1 << 20) || !r) return KZGPOT_E_INVALID_ARG;
  switch (op) {
    case KZGPOT_F30_MUL: return run_op<KZGPOT_F30_MUL>(n, a, b, c, d, r);
    case KZGPOT_F30_SQR: return run_op<KZGPOT_F30_SQR>(n, a, b, c, d, r);
    case KZGPOT_F30_MUL_ADDSQR: return run_op<KZGPOT_F30_MUL_ADDSQR>(n, a, b, c, d, r);
    case KZGPOT_F30_MUL_SUM2: return run_op<KZGPOT_F30_MUL_SUM2>(n, a, b, c, d, r);
    case KZGPOT_F30_DBL: return run_op<KZGPOT_F30_DBL>(n, a, b, c, d, r);
    case KZGPOT_F30_MUL3: return run_op<KZGPOT_F30_MUL3>(n, a, b, c, d, r);
    case KZGPOT_F30_NORM0: return run_op<KZGPOT_F30_NORM0>(n, a, b, c, d, r);
    case KZGPOT_F30_NORM1: return run_op<KZGPOT_F30_NORM1>(n, a, b, c, d, r);
    case KZGPOT_F30_NORM2: return run_op<KZGPOT_F30_NORM2>(n, a, b, c, d, r);
    case KZGPOT_F30_NORM3: return run_op<KZGPOT_F30_NORM3>(n, a, b, c, d, r);
    default: return KZGPOT_E_INVALID_ARG;
  }
}
#endif  // KZGPOT_TEST_HOOKS
