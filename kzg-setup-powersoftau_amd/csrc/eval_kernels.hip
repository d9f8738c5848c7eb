// Fr vectors in evaluation form: the batch inversion, and the division of a
// polynomial by (x - z) from its n = 2^exp evaluations e_i = p(w^i), natural order.
//
// Batch inversion (Montgomery's trick inside a tile). A block of 256 lanes owns a tile of S = 2^t
// entries, a lane a run of M = S / 256 consecutive ones, staged through LDS as poly_parts.hpp states:
//   1  lane: the prefix products of its run; the product before entry k stays in registers. A zero
//      entry counts as 1 and is remembered in a bit mask, so no product is ever zero.
//   2  block: a prefix scan and a suffix scan over the 256 run products (8 steps each, written out
//      in tile_invert, which says why they are not poly_parts.hpp's block_scan) give lane l the
//      product E of the runs before it and the product X of the runs behind it.
//   3  lane 255 holds the tile's product and inverts it: the one inversion of the tile, 512 dependent
//      binary steps (fr_inv_binary, csrc/fr.hpp) in one lane of one wave while the other three wait.
//   4  E X / (the tile's product) is the inverse of the lane's own run product; the back-sweep over
//      the run multiplies it by the product before entry k (the inverse of entry k) and then by
//      entry k itself. Remembered zeros come out as zeros.
// One inversion per tile and no dependency between blocks: no grid-wide synchronisation, no
// look-back, no spin-wait, no cooperative launch. Five multiplications per entry (load, prefix, two
// in the back-sweep, store) and 18 per lane.
//
// Division in evaluation form, for z off the domain (z^n != 1) and on it (z = w^m):
//   k_eval_inv<t>   per tile: w^i from the powers w^(2^k) (one ladder per lane, then a step of w along
//                   the run), the differences z - w^i inverted by the routine above (the lane that
//                   meets the zero difference stores its index m: at most one does), inv_i to the
//                   workspace, and the tile's share of  sum_i e_i w^i inv_i = z sum_i e_i inv_i - sum_i e_i
//                   (w^i / (z - w^i) = z / (z - w^i) - 1, so the second pass needs no power of w)
//   k_eval_value    one block: value = (z^n - 1) / n times the sum of the shares, or e_m
//   k_eval_quot<t>  q_i = (value - e_i) inv_i, canonical; with m set also the tile's share of
//                   sum_i q_i w^(i-m) (inv_m is 0, so q_m = 0 takes no part)
//   k_eval_fix      one block, with m set: q_m = - sum_{i != m} q_i w^(i-m)
// The workspace and the tile counts are eval_plan's (plans.hpp). Values are Montgomery (R = 2^256)
// between load and store; the workspace's inv_i stay in that form.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "codec.hpp"
#include "poly_parts.hpp"

namespace kzgpot {
namespace {

// M values of one lane in registers. The index is the same for every lane of a wave and every
// access a chain of selects over the M slots: an array indexed by the loop counter would live in
// scratch, and unrolling the sweeps instead is M copies of their multiplications.
template <int M, class = std::make_integer_sequence<int, M>>
struct RunRegs;
template <int M, int... Q>
struct RunRegs<M, std::integer_sequence<int, Q...>> {
  fr v[M];
  static __device__ inline void pick(fr& out, bool c, const fr& a) {  // word by word: no select between addresses
#pragma unroll
    for (int j = 0; j < 8; j++) out.v[j] = c ? a.v[j] : out.v[j];
  }
  __device__ inline void set(int k, const fr& a) { (pick(v[Q], Q == k, a), ...); }
  __device__ inline fr get(int k) const {
    fr a = v[0];
    (pick(a, Q == k, v[Q]), ...);
    return a;
  }
};

// The lane's run in the tile -> the inverse of each entry, zero for a zero. RAW: the entries are any
// 256-bit integers and the inverses leave canonical; otherwise both are in Montgomery form. Every
// lane of the block calls it; rows is free on entry and on return.
template <int T, bool RAW>
__device__ inline void tile_invert(uint4* tile, uint32_t (*rows)[256]) {
  using G = Tile<T>;
  constexpr int PAIRS = G::M / 2;
  const uint32_t tid = threadIdx.x;
  const int s = (int)tid * G::RUN;
  // entry k of the run, a zero taken as 1 and remembered
  uint32_t zeros = 0;
  auto entry = [&](int k) {
    fr a;
    get_entry(a, tile, s + 2 * k);
    if (RAW) fr_load(a, a);
    const bool zero = fr_is_zero(a);
    if (zero) {
      zeros |= 1u << k;
      a = fr_one();
    }
    if (RAW || zero) put_entry(tile, s + 2 * k, a);
    return a;
  };
  auto leave = [&](int k, fr o) {
    if (RAW) fr_store(o, o);
    if ((zeros >> k) & 1) o = fr_zero();
    put_entry(tile, s + 2 * k, o);
  };
  // the product of the run's entries before each pair (2 p, 2 p + 1); the product before the odd
  // entry is one multiplication away, which halves what the back-sweep needs from registers
  RunRegs<PAIRS ? PAIRS : 1> before;
  fr run;
  if constexpr (PAIRS == 0) {
    run = entry(0);
  } else {
    run = fr_one();
#pragma unroll 1
    for (int p = 0; p < PAIRS; p++) {
      before.set(p, run);
      fr_mul(run, run, entry(2 * p));
      fr_mul(run, run, entry(2 * p + 1));
    }
  }
  // The two scans are written out here, not poly_parts.hpp's block_scan: through the shared loop the
  // batch inversion at the library's tile measured 1 - 2 % slower in two alternating A/B runs (the
  // scan bodies' mad chains come out in another order; profiles/r14_ab_fr_parts.json), so this
  // routine keeps the parent's text and, with it, the parent's code.
  // the runs behind this lane's: after step k lane l holds the product of the runs [l, l + 2^(k+1))
  fr acc = run, nb;
  park(rows, tid, acc);
#pragma unroll 1
  for (int k = 0; k < 8; k++) {
    const uint32_t d = 1u << k;
    __syncthreads();
    if (tid + d < 256) unpark(nb, rows, tid + d);
    __syncthreads();
    if (tid + d < 256) {
      fr_mul(acc, acc, nb);
      park(rows, tid, acc);
    }
  }
  __syncthreads();
  fr inv = fr_one();
  if (tid < 255) unpark(inv, rows, tid + 1);
  __syncthreads();
  // the runs before it, from the other end: (l - 2^(k+1), l]; lane 255 ends with the tile's product
  acc = run;
  park(rows, tid, acc);
#pragma unroll 1
  for (int k = 0; k < 8; k++) {
    const uint32_t d = 1u << k;
    __syncthreads();
    if (tid >= d) unpark(nb, rows, tid - d);
    __syncthreads();
    if (tid >= d) {
      fr_mul(acc, acc, nb);
      park(rows, tid, acc);
    }
  }
  __syncthreads();
  if (tid > 0) {
    unpark(nb, rows, tid - 1);
    fr_mul(inv, inv, nb);
  }
  __syncthreads();
  if (tid == 255) park(rows, 0, fr_inv_binary(acc));  // the one inversion of the tile
  __syncthreads();
  unpark(nb, rows, 0);
  fr_mul(inv, inv, nb);  // 1 / (the run's product)
  __syncthreads();
  if constexpr (PAIRS == 0) {
    leave(0, inv);
  } else {
#pragma unroll 1
    for (int p = PAIRS - 1; p >= 0; p--) {
      fr a0, a1, o0, o1;
      get_entry(a0, tile, s + 4 * p);
      get_entry(a1, tile, s + 4 * p + 2);
      const fr b0 = before.get(p);
      fr_mul(o1, b0, a0);  // the product before the odd entry
      fr_mul(o1, o1, inv);
      fr_mul(inv, inv, a1);
      fr_mul(o0, b0, inv);
      fr_mul(inv, inv, a0);
      leave(2 * p, o0);
      leave(2 * p + 1, o1);
    }
  }
}

// the padded tile -> entries [blk S, (blk + 1) S) of out, those below n
template <int T>
__device__ inline void stage_out(uint4* out, const uint4* tile, uint64_t blk, uint64_t n) {
  using G = Tile<T>;
  const uint64_t base = blk * (2 * G::S), end = 2 * n;
#pragma unroll
  for (int r = 0; r < 2 * G::M; r++) {
    const int i = r * 256 + (int)threadIdx.x;
    const uint64_t g = base + (uint64_t)i;
    if (g < end) out[g] = tile[i + (i >> (G::LOG2M + 1))];
  }
}

// ---------------------------------------------------------------- batch inversion
// out may be in: a block reads its own tile, then writes it
template <int T>
__global__ void __launch_bounds__(256) k_fr_batch_inverse(const uint4* in, uint64_t n, uint4* out) {
  using G = Tile<T>;
  __shared__ uint4 tile[G::SLOTS];
  __shared__ uint32_t rows[8][256];
  stage_in<T>(tile, in, blockIdx.x, n);  // zeros past the end: skipped like any zero
  __syncthreads();
  tile_invert<T, true>(tile, rows);
  __syncthreads();
  stage_out<T>(out, tile, blockIdx.x, n);
}

// ---------------------------------------------------------------- division in evaluation form
template <int T>
__global__ void __launch_bounds__(256) k_eval_inv(const uint4* __restrict__ evals, uint64_t n, uint4* __restrict__ inv,
                                                  uint32_t* __restrict__ sums, uint32_t* __restrict__ m_word,
                                                  fr_eval_scalars sc) {
  using G = Tile<T>;
  __shared__ uint4 tile[G::SLOTS];
  __shared__ uint32_t rows[8][256];
  const uint32_t tid = threadIdx.x;
  const uint64_t blk = blockIdx.x, i0 = blk * G::S + (uint64_t)tid * G::M;
  const int s = (int)tid * G::RUN;
  fr w = power_from_table<kEvalPowers>(sc.pw, i0, fr_one());
#pragma unroll 1
  for (int k = 0; k < G::M; k++) {
    const uint64_t i = i0 + (uint64_t)k;
    fr d;
    fr_sub(d, sc.z, w);
    if (i >= n) d = fr_one();  // past the domain (n < S): w^i has wrapped round
    else if (fr_is_zero(d)) *m_word = (uint32_t)i;
    put_entry(tile, s + 2 * k, d);
    fr_mul(w, w, sc.pw[0]);
  }
  tile_invert<T, false>(tile, rows);
  __syncthreads();
  stage_out<T>(inv, tile, blk, n);
  // entries tid, tid + 256, ..: e_i read where it lies, inv_i from the tile
  fr by_inv = fr_zero(), plain = fr_zero();
#pragma unroll 1
  for (int r = 0; r < G::M; r++) {
    const int j = r * 256 + (int)tid;
    const uint64_t i = blk * G::S + (uint64_t)j;
    if (i < n) {
      fr e, v;
      load_entry(e, evals, i);
      get_entry(v, tile, 2 * j + (j >> G::LOG2M));
      mul_add(by_inv, e, v, by_inv);
      fr_add(plain, plain, e);
    }
  }
  fr acc;
  fr_mul(acc, by_inv, sc.z);
  fr_sub(acc, acc, plain);
  block_sum(acc, rows);
  if (tid == 0) words_out(sums + blk * 8, acc);
}

__global__ void __launch_bounds__(256) k_eval_value(const uint32_t* __restrict__ sums, uint64_t tiles,
                                                    const uint4* __restrict__ evals, const uint32_t* __restrict__ m_word,
                                                    uint32_t* __restrict__ value, fr scale) {
  __shared__ uint32_t rows[8][256];
  fr acc;
  sum_entries(acc, sums, tiles, rows);
  if (threadIdx.x) return;
  const uint32_t m = *m_word;
  if (m != kEvalNoIndex) load_entry(acc, evals, m);
  else fr_mul(acc, acc, scale);
  fr_store(acc, acc);
  words_out(value, acc);
}

// quot must not overlap evals
template <int T>
__global__ void __launch_bounds__(256) k_eval_quot(const uint4* __restrict__ evals, uint64_t n,
                                                   const uint4* __restrict__ inv, const uint32_t* __restrict__ value,
                                                   const uint32_t* __restrict__ m_word, uint4* __restrict__ quot,
                                                   uint32_t* __restrict__ qsums, fr_eval_scalars sc) {
  using G = Tile<T>;
  __shared__ uint32_t rows[8][256];
  const uint32_t tid = threadIdx.x;
  const uint64_t blk = blockIdx.x;
  const uint32_t m = *m_word;
  const bool on = m != kEvalNoIndex;  // the same for every lane of the grid
  fr v, w = fr_one(), acc = fr_zero();
  words_in(v, value);
  fr_load(v, v);
  // w^(i - m), i = blk S + tid
  if (on) w = power_from_table<kEvalPowers>(sc.pw, (blk * G::S + tid + n - m) & (n - 1), fr_one());
#pragma unroll 1
  for (int r = 0; r < G::M; r++) {
    const uint64_t i = blk * G::S + (uint64_t)(r * 256) + tid;
    if (i < n) {
      fr e, vi, q;
      load_entry(e, evals, i);
      get_entry(vi, inv, 2 * i);
      fr_sub(e, v, e);
      fr_mul(q, e, vi);
      if (on) mul_add(acc, q, w, acc);
      store_entry(quot, i, q);
    }
    if (on) fr_mul(w, w, sc.pw[8]);  // 256 entries on
  }
  if (!on) return;
  block_sum(acc, rows);
  if (tid == 0) words_out(qsums + blk * 8, acc);
}

__global__ void __launch_bounds__(256) k_eval_fix(const uint32_t* __restrict__ qsums, uint64_t tiles,
                                                  const uint32_t* __restrict__ m_word, uint32_t* __restrict__ quot) {
  __shared__ uint32_t rows[8][256];
  const uint32_t m = *m_word;
  if (m == kEvalNoIndex) return;
  fr acc;
  sum_entries(acc, qsums, tiles, rows);
  if (threadIdx.x) return;
  fr_sub(acc, fr_zero(), acc);
  fr_store(acc, acc);
  words_out(quot + (uint64_t)m * 8, acc);
}

template <int T>
hipError_t launch_inverse(const void* d_in, uint64_t n, void* d_out, hipStream_t s) {
  hipLaunchKernelGGL(k_fr_batch_inverse<T>, dim3((unsigned)batch_inverse_tiles(n, T)), dim3(256), 0, s, (const uint4*)d_in,
                     n, (uint4*)d_out);
  return hipGetLastError();
}

template <int T>
hipError_t launch_divide(const EvalPlan& p, const void* d_evals, const fr_eval_scalars& sc, void* d_quotient,
                         void* d_value, void* d_work, hipStream_t s) {
  uint8_t* w = (uint8_t*)d_work;
  uint32_t *sums = (uint32_t*)(w + p.sums), *qsums = (uint32_t*)(w + p.qsums), *m_word = (uint32_t*)(w + p.words);
  uint4* inv = (uint4*)(w + p.inv);
  const uint4* evals = (const uint4*)d_evals;
  const dim3 tiles((unsigned)p.tiles), one(1), block(256);
  if (const hipError_t e = hipMemsetAsync(m_word, 0xff, 4, s)) return e;
  hipLaunchKernelGGL(k_eval_inv<T>, tiles, block, 0, s, evals, p.n, inv, sums, m_word, sc);
  hipLaunchKernelGGL(k_eval_value, one, block, 0, s, sums, p.tiles, evals, m_word, (uint32_t*)d_value, sc.scale);
  if (d_quotient) {
    hipLaunchKernelGGL(k_eval_quot<T>, tiles, block, 0, s, evals, p.n, inv, (const uint32_t*)d_value, m_word,
                       (uint4*)d_quotient, qsums, sc);
    hipLaunchKernelGGL(k_eval_fix, one, block, 0, s, qsums, p.tiles, m_word, (uint32_t*)d_quotient);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_fr_batch_inverse(const void* d_in, uint64_t n, void* d_out, uint32_t t, hipStream_t stream) {
  if (!n) return hipSuccess;
  if (!batch_inverse_tiles(n, t)) return hipErrorInvalidValue;
  return with_tile<kPolyTileMin, kPolyTileMax>(t, [&](auto T) { return launch_inverse<T()>(d_in, n, d_out, stream); });
}

hipError_t launch_evals_divide(const EvalPlan& p, const void* d_evals, const fr_eval_scalars& sc, void* d_quotient,
                               void* d_value, void* d_work, hipStream_t stream) {
  if (!p.bytes) return hipErrorInvalidValue;
  return with_tile<kPolyTileMin, kPolyTileMax>(
      p.t, [&](auto T) { return launch_divide<T()>(p, d_evals, sc, d_quotient, d_value, d_work, stream); });
}

}  // namespace kzgpot
