// Test build only (libkzgpot_test.so, -DKZGPOT_TEST_HOOKS; tests/kzgpot_test_fp_hooks.h): one function of
// the 14 x 28 / 9 x 29 limb core (fp381.hpp fp_*, the Fp2 f_mul / f_sqr, the 14 x 28 <-> 13 x 30
// conversions, f30_is_zero<F30_ZK>) per lane on caller-supplied limb arrays, so that
// tests/test_gpu_fp28_core.py can compare the functions' output LIMBS with an exact integer model —
// the codec tests see only canonical bytes: they cannot hand a multiply a loose limb, a zero test a
// nonzero value that passes its filter, or a borrowed-constant form a limb at its dominance bound.
#ifdef KZGPOT_TEST_HOOKS
#include "../../tests/kzgpot_test_fp_hooks.h"
#include "curve.hpp"
#include "device_rt.hpp"

using namespace kzgpot;

namespace {

constexpr int kBlock = 256;

constexpr bool is_kb(int op) { return op >= KZGPOT_FP_SUBK && op < KZGPOT_FP_NEGK + KZGPOT_FP_KB_COUNT; }
constexpr bool is_pred(int op) {
  return op == KZGPOT_FP_IS_ZERO || op == KZGPOT_FP_EQ || op == KZGPOT_FP_LT_CANON || op == KZGPOT_FP_F30_IS_ZERO;
}
constexpr bool f30_in(int op) {
  return op == KZGPOT_FP_F30_IS_ZERO || op == KZGPOT_FP_FROM_F30 || op == KZGPOT_FP_MONT_FROM_F30_1 ||
         op == KZGPOT_FP_MONT_FROM_F30_2;
}
constexpr bool f30_out(int op) {
  return op == KZGPOT_FP_F30_FROM_FP || op == KZGPOT_FP_F30_FROM_MONT1 || op == KZGPOT_FP_F30_FROM_MONT2;
}
constexpr int arity(int op) {
  if (is_kb(op)) return op >= KZGPOT_FP_NEGK ? 1 : 2;
  switch (op) {
    case KZGPOT_FP_MUL_SUM3: return 6;
    case KZGPOT_FP_MUL_SUM2:
    case KZGPOT_FP_F2_MUL: return 4;
    case KZGPOT_FP_MUL_ADDSQR8: return 3;
    case KZGPOT_FP_MUL:
    case KZGPOT_FP_EQ:
    case KZGPOT_FP_LT_CANON:
    case KZGPOT_FP_ADD_RED:
    case KZGPOT_FP_SUB_RED:
    case KZGPOT_FP_F2_SQR:
    case KZGPOT_FP_ADD: return 2;
    default: return 1;
  }
}
// words per lane of an operand and of the result
template <class Tr>
constexpr int in_width(int op) {
  return op == KZGPOT_FP_FROM_WORDS ? Tr::NW : f30_in(op) ? N30 : Tr::NL;
}
template <class Tr>
constexpr int out_width(int op) {
  return is_pred(op)                                         ? 1
         : op == KZGPOT_FP_TO_WORDS                          ? Tr::NW
         : f30_out(op)                                       ? N30
         : op == KZGPOT_FP_F2_MUL || op == KZGPOT_FP_F2_SQR ? 2 * Tr::NL
                                                             : Tr::NL;
}

template <class Tr>
__device__ __forceinline__ void fe_load(Fe<Tr>& x, const uint32_t* p, long i) {
#pragma unroll
  for (int k = 0; k < Tr::NL; k++) x.v[k] = p[Tr::NL * i + k];
}
template <class Tr>
__device__ __forceinline__ void fe_store(uint32_t* p, long i, int stride, int at, const Fe<Tr>& x) {
#pragma unroll
  for (int k = 0; k < Tr::NL; k++) p[stride * i + at + k] = x.v[k];
}

template <int OP, class Tr>
__global__ void __launch_bounds__(kBlock) k_fp_op(long n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                  const uint32_t* __restrict__ c, const uint32_t* __restrict__ d,
                                                  const uint32_t* __restrict__ e, const uint32_t* __restrict__ f,
                                                  uint32_t* __restrict__ r) {
  const long i = (long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;  // before the call: the zero tests' ballots also run in a wave with inactive lanes
  constexpr int N = Tr::NL;
  constexpr bool bls = __is_same(Tr, BlsFp);
  if constexpr (OP == KZGPOT_FP_FROM_WORDS) {
    uint32_t w[Tr::NW];
#pragma unroll
    for (int k = 0; k < Tr::NW; k++) w[k] = a[Tr::NW * i + k];
    Fe<Tr> o;
    fp_from_words(o, w);
    fe_store(r, i, N, 0, o);
  } else if constexpr (f30_in(OP)) {
    static_assert(bls, "the radix-2^30 core is BLS12-381's");
    f30 z;
#pragma unroll
    for (int k = 0; k < N30; k++) z.v[k] = (int32_t)a[N30 * i + k];
    if constexpr (OP == KZGPOT_FP_F30_IS_ZERO) {
      r[i] = f30_is_zero<F30_ZK>(z) ? 1u : 0u;
    } else {
      fp o;
      if (OP == KZGPOT_FP_FROM_F30) fp_from_f30(o, z);
      if (OP == KZGPOT_FP_MONT_FROM_F30_1) fp_mont_from_f30<1>(o, z);
      if (OP == KZGPOT_FP_MONT_FROM_F30_2) fp_mont_from_f30<2>(o, z);
      fe_store(r, i, N, 0, o);
    }
  } else {
    Fe<Tr> x[6], o;
    const uint32_t* in[6] = {a, b, c, d, e, f};
#pragma unroll
    for (int k = 0; k < arity(OP); k++) fe_load(x[k], in[k], i);
    if constexpr (is_pred(OP)) {
      bool p = false;
      if (OP == KZGPOT_FP_IS_ZERO) p = fp_is_zero(x[0]);
      if (OP == KZGPOT_FP_EQ) p = fp_eq(x[0], x[1]);
      if (OP == KZGPOT_FP_LT_CANON) p = fp_lt_canon(x[0], x[1]);
      r[i] = p ? 1u : 0u;
    } else if constexpr (OP == KZGPOT_FP_TO_WORDS) {
      uint32_t w[Tr::NW];
      fp_to_words(w, x[0]);
#pragma unroll
      for (int k = 0; k < Tr::NW; k++) r[Tr::NW * i + k] = w[k];
    } else if constexpr (f30_out(OP)) {
      static_assert(bls, "the radix-2^30 core is BLS12-381's");
      f30 z;
      if (OP == KZGPOT_FP_F30_FROM_FP) f30_from_fp(z, x[0]);
      if (OP == KZGPOT_FP_F30_FROM_MONT1) f30_from_mont<1>(z, x[0]);
      if (OP == KZGPOT_FP_F30_FROM_MONT2) f30_from_mont<2>(z, x[0]);
#pragma unroll
      for (int k = 0; k < N30; k++) r[N30 * i + k] = (uint32_t)z.v[k];
    } else if constexpr (OP == KZGPOT_FP_F2_MUL || OP == KZGPOT_FP_F2_SQR) {
      static_assert(bls, "Fp2 is BLS12-381's");
      fp2 u{x[0], x[1]}, v{x[2], x[3]}, w;
      if (OP == KZGPOT_FP_F2_MUL) f_mul(w, u, v);
      if (OP == KZGPOT_FP_F2_SQR) f_sqr(w, u);
      fe_store(r, i, 2 * N, 0, w.c0);
      fe_store(r, i, 2 * N, N, w.c1);
    } else {
      if constexpr (OP == KZGPOT_FP_MUL) fp_mul(o, x[0], x[1]);
      if constexpr (OP == KZGPOT_FP_SQR) fp_sqr(o, x[0]);
      if constexpr (OP == KZGPOT_FP_MUL_SUM2) fp_mul_sum2(o, x[0], x[1], x[2], x[3]);
      if constexpr (OP == KZGPOT_FP_MUL_SUM3) fp_mul_sum3(o, x[0], x[1], x[2], x[3], x[4], x[5]);
      if constexpr (OP == KZGPOT_FP_MUL_ADDSQR8) fp_mul_add8sqr(o, x[0], x[1], x[2]);
      if constexpr (OP == KZGPOT_FP_NORM) fp_norm(o, x[0]);
      if constexpr (OP == KZGPOT_FP_HALF) fp_half(o, x[0]);
      if constexpr (OP == KZGPOT_FP_REDUCE_ONCE) fp_reduce_once(o, x[0]);
      if constexpr (OP == KZGPOT_FP_REDUCE_CANON) fp_reduce_canon(o, x[0]);
      if constexpr (OP == KZGPOT_FP_CANON) fp_canon(o, x[0]);
      if constexpr (OP == KZGPOT_FP_NEG_CANON) fp_neg_canon(o, x[0]);
      if constexpr (OP == KZGPOT_FP_COND_SUB_2P) fp_cond_sub_2p(o, x[0]);
      if constexpr (OP == KZGPOT_FP_ADD_RED) fp_add_red(o, x[0], x[1]);
      if constexpr (OP == KZGPOT_FP_SUB_RED) fp_sub_red(o, x[0], x[1]);
      if constexpr (OP == KZGPOT_FP_TO_MONT) fp_to_mont(o, x[0]);
      if constexpr (OP == KZGPOT_FP_FROM_MONT) fp_from_mont(o, x[0]);
      if constexpr (OP == KZGPOT_FP_ADD) fp_add(o, x[0], x[1]);
#define KZG_KB_OP(idx, name)                                                            \
  if constexpr (OP == KZGPOT_FP_SUBK + idx) fp_subk_nr<Tr::name>(o, x[0], x[1]); \
  if constexpr (OP == KZGPOT_FP_NEGK + idx) fp_negk_nr<Tr::name>(o, x[0]);
      KZGPOT_FP_KB_LIST(KZG_KB_OP)
#undef KZG_KB_OP
      fe_store(r, i, N, 0, o);
    }
  }
}

template <int OP, class Tr>
int run_op(long n, const uint32_t* const (&in)[6], uint32_t* r) {
  constexpr int n_in = arity(OP);
  for (int k = 0; k < n_in; k++)
    if (!in[k]) return KZGPOT_E_INVALID_ARG;
  if (device_count() <= 0) return KZGPOT_E_DEVICE;
  const size_t in_bytes = (size_t)n * in_width<Tr>(OP) * sizeof(uint32_t);
  const size_t out_bytes = (size_t)n * out_width<Tr>(OP) * sizeof(uint32_t);
  DevBuf din[6], dout;
  for (int k = 0; k < n_in; k++) {
    if (din[k].alloc(in_bytes)) return KZGPOT_E_DEVICE;
    HIP_TRY(hipMemcpy(din[k].p, in[k], in_bytes, hipMemcpyHostToDevice));
  }
  if (dout.alloc(out_bytes)) return KZGPOT_E_DEVICE;
  const unsigned blocks = (unsigned)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL((k_fp_op<OP, Tr>), dim3(blocks), dim3(kBlock), 0, nullptr, n, (const uint32_t*)din[0].p,
                     (const uint32_t*)din[1].p, (const uint32_t*)din[2].p, (const uint32_t*)din[3].p,
                     (const uint32_t*)din[4].p, (const uint32_t*)din[5].p, (uint32_t*)dout.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(nullptr));
  HIP_TRY(hipMemcpy(r, dout.p, out_bytes, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" int kzgpot_test_fp_op(int op, int field, long n, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                 const uint32_t* d, const uint32_t* e, const uint32_t* f, uint32_t* r) {
  if (n <= 0 || n > (1 << 20) || !r || (field != KZGPOT_FP_BLS && field != KZGPOT_FP_BN254)) return KZGPOT_E_INVALID_ARG;
  const uint32_t* const in[6] = {a, b, c, d, e, f};
  const bool bn = field == KZGPOT_FP_BN254;
#define KZG_BOTH(OP) \
  case OP: return bn ? run_op<OP, Bn254Fp>(n, in, r) : run_op<OP, BlsFp>(n, in, r);
#define KZG_BLS(OP) \
  case OP: return bn ? KZGPOT_E_INVALID_ARG : run_op<OP, BlsFp>(n, in, r);
#define KZG_KB_CASE(idx, name)                                                       \
  case KZGPOT_FP_SUBK + idx:                                                         \
    if (bn) return idx == KZGPOT_FP_KB_EQ_INDEX ? run_op<KZGPOT_FP_SUBK + KZGPOT_FP_KB_EQ_INDEX, Bn254Fp>(n, in, r) \
                                                : KZGPOT_E_INVALID_ARG;              \
    return run_op<KZGPOT_FP_SUBK + idx, BlsFp>(n, in, r);                            \
  case KZGPOT_FP_NEGK + idx:                                                         \
    if (bn) return idx == KZGPOT_FP_KB_EQ_INDEX ? run_op<KZGPOT_FP_NEGK + KZGPOT_FP_KB_EQ_INDEX, Bn254Fp>(n, in, r) \
                                                : KZGPOT_E_INVALID_ARG;              \
    return run_op<KZGPOT_FP_NEGK + idx, BlsFp>(n, in, r);
  switch (op) {
    KZG_BOTH(KZGPOT_FP_MUL)
    KZG_BOTH(KZGPOT_FP_SQR)
    KZG_BLS(KZGPOT_FP_MUL_SUM2)
    KZG_BLS(KZGPOT_FP_MUL_SUM3)
    KZG_BLS(KZGPOT_FP_MUL_ADDSQR8)
    KZG_BLS(KZGPOT_FP_NORM)
    KZG_BLS(KZGPOT_FP_HALF)
    KZG_BLS(KZGPOT_FP_REDUCE_ONCE)
    KZG_BLS(KZGPOT_FP_REDUCE_CANON)
    KZG_BLS(KZGPOT_FP_CANON)
    KZG_BOTH(KZGPOT_FP_IS_ZERO)
    KZG_BOTH(KZGPOT_FP_EQ)
    KZG_BOTH(KZGPOT_FP_LT_CANON)
    KZG_BOTH(KZGPOT_FP_NEG_CANON)
    KZG_BLS(KZGPOT_FP_COND_SUB_2P)
    KZG_BLS(KZGPOT_FP_ADD_RED)
    KZG_BLS(KZGPOT_FP_SUB_RED)
    KZG_BLS(KZGPOT_FP_F2_MUL)
    KZG_BLS(KZGPOT_FP_F2_SQR)
    KZG_BOTH(KZGPOT_FP_FROM_WORDS)
    KZG_BOTH(KZGPOT_FP_TO_WORDS)
    KZG_BOTH(KZGPOT_FP_TO_MONT)
    KZG_BOTH(KZGPOT_FP_FROM_MONT)
    KZG_BOTH(KZGPOT_FP_ADD)
    KZG_BLS(KZGPOT_FP_F30_IS_ZERO)
    KZG_BLS(KZGPOT_FP_F30_FROM_FP)
    KZG_BLS(KZGPOT_FP_FROM_F30)
    KZG_BLS(KZGPOT_FP_F30_FROM_MONT1)
    KZG_BLS(KZGPOT_FP_F30_FROM_MONT2)
    KZG_BLS(KZGPOT_FP_MONT_FROM_F30_1)
    KZG_BLS(KZGPOT_FP_MONT_FROM_F30_2)
    KZGPOT_FP_KB_LIST(KZG_KB_CASE)
    default: return KZGPOT_E_INVALID_ARG;
  }
#undef KZG_BOTH
#undef KZG_BLS
#undef KZG_KB_CASE
}
#endif  // KZGPOT_TEST_HOOKS
