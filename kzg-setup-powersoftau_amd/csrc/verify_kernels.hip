// KZG10 check / batch_check, the kernels around the two MSMs and the pairing product (DESIGN.md §14;
// verify.hip enqueues them, check_plan in plans.hpp lays out what they read and write).
//
//   k_check_scalars  a block of 256 lanes owns 256 proofs, a lane one: rho_i, z_i, v_i and vbar_i are
//                    any 256-bit integers, loaded as their residues. It writes the MSM's scalar rows
//                    rho_i (row i) and rho_i z_i (row n + i), canonical, and the block's shares of
//                    sum rho_i v_i and sum rho_i vbar_i (block_sum; it and the entry accessors are
//                    poly_parts.hpp's)
//   k_check_sums     one block: the sums of the shares, negated, as the scalars of g and gamma_g
//                    (rows 2 n and 2 n + 1)
//   k_g1_negate      one lane: an ark G1 record -> the record of its negative (infinity stays)
// Values are Montgomery (R = 2^256) between load and store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec.hpp"
#include "group_parts.hpp"
#include "poly_parts.hpp"

namespace kzgpot {
namespace {

// random_vs may be null (no proof is hiding: every vbar_i is 0)
__global__ void __launch_bounds__(256) k_check_scalars(const uint4* __restrict__ randomizers, const uint4* __restrict__ points,
                                                       const uint4* __restrict__ values, const uint4* __restrict__ random_vs,
                                                       uint64_t n, uint4* __restrict__ scalars, uint32_t* __restrict__ sums,
                                                       uint64_t blocks) {
  __shared__ uint32_t rows[8][256];
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  fr sv = fr_zero(), sb = fr_zero();
  if (i < n) {
    fr rho, x;
    load_entry(rho, randomizers, i);
    store_entry(scalars, i, rho);
    load_entry(x, points, i);
    fr_mul(x, x, rho);
    store_entry(scalars, n + i, x);
    load_entry(x, values, i);
    fr_mul(sv, x, rho);
    if (random_vs) {
      load_entry(x, random_vs, i);
      fr_mul(sb, x, rho);
    }
  }
  block_sum(sv, rows);
  block_sum(sb, rows);
  if (threadIdx.x == 0) {
    words_out(sums + (uint64_t)blockIdx.x * 8, sv);
    words_out(sums + (blocks + blockIdx.x) * 8, sb);
  }
}

__global__ void __launch_bounds__(256) k_check_sums(const uint32_t* __restrict__ sums, uint64_t blocks, uint64_t n,
                                                    uint4* __restrict__ scalars) {
  __shared__ uint32_t rows[8][256];
  fr sv, sb;
  sum_entries(sv, sums, blocks, rows);
  sum_entries(sb, sums + blocks * 8, blocks, rows);
  if (threadIdx.x) return;
  fr_sub(sv, fr_zero(), sv);
  fr_sub(sb, fr_zero(), sb);
  store_entry(scalars, 2 * n, sv);
  store_entry(scalars, 2 * n + 1, sb);
}

// in place; the record is the MSM's own output (or zeros where the MSM rejected a base and wrote nothing)
__global__ void __launch_bounds__(64) k_g1_negate(uint4* rec) {
  if (threadIdx.x) return;
  fp x, y;
  bool inf;
  if (ark_record_decode(x, y, inf, rec) || inf) return;
  fp_from_mont(y, y);
  fp_neg_canon(y, y);
  store_canon(rec + 3, y);
}

}  // namespace

hipError_t launch_check_scalars(const CheckPlan& p, const void* d_randomizers, const void* d_points, const void* d_values,
                                const void* d_random_vs, void* d_work, hipStream_t stream) {
  uint8_t* w = (uint8_t*)d_work;
  uint4* scalars = (uint4*)(w + p.scalars);
  uint32_t* sums = (uint32_t*)(w + p.sums);
  hipLaunchKernelGGL(k_check_scalars, dim3((unsigned)p.blocks), dim3(256), 0, stream, (const uint4*)d_randomizers,
                     (const uint4*)d_points, (const uint4*)d_values, (const uint4*)d_random_vs, p.n, scalars, sums, p.blocks);
  hipLaunchKernelGGL(k_check_sums, dim3(1), dim3(256), 0, stream, (const uint32_t*)sums, p.blocks, p.n, scalars);
  return hipGetLastError();
}

hipError_t launch_g1_negate(void* d_record, hipStream_t stream) {
  hipLaunchKernelGGL(k_g1_negate, dim3(1), dim3(64), 0, stream, (uint4*)d_record);
  return hipGetLastError();
}

}  // namespace kzgpot
