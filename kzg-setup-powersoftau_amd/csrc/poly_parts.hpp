// What the kernels over Fr vectors share, each idiom stated once (poly_kernels.hip: the polynomial
// division; eval_kernels.hip: the batch inversion and the division in evaluation form;
// ntt_kernels.hip: the NTT; verify_kernels.hip: the check's Fr pass; fft_kernels.hip: the twiddles):
//   entries   an fr as two uint4 (HBM or LDS) and as eight words, raw or through Montgomery form
//   columns   park / unpark: word-major LDS rows, one value per lane or slot
//   block     block_tree and block_scan: the eight-step loops over the 256 lanes' values with their
//             barriers (eval_kernels.hip's tile_invert alone keeps its two product scans written
//             out, for the measured reason it states); scan_neighbour reads a scan's result
//   powers    power_from_table: x^e from the squarings x^(2^k)
//   tiles     the padded-run tile and with_tile, a runtime tile width -> its kernel instantiation
//
// The tile: a block of 256 lanes owns S = 2^T entries of 32 B, a lane a run of M = S / 256
// consecutive entries. Global loads and stores are one uint4 per lane at consecutive addresses; in
// LDS a run takes 2 M + 1 uint4 (one of padding: an odd stride, so the 16-byte accesses of
// neighbouring lanes fall into different banks). `rows` is a lane's column of one value per lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "fr.hpp"

namespace kzgpot {
namespace {

// ---------------------------------------------------------------- entries
// the 32 bytes at v[slot], v[slot + 1] (HBM or LDS) <-> the eight words as they are
template <class I>
__device__ inline void get_entry(fr& a, const uint4* v, I slot) {
  const uint4 lo = v[slot], hi = v[slot + 1];
  a = fr{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
}
template <class I>
__device__ inline void put_entry(uint4* v, I slot, const fr& a) {
  v[slot] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
  v[slot + 1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}
// entry i of v: any 256-bit integer -> Montgomery form, and Montgomery form -> the canonical value
__device__ inline void load_entry(fr& a, const uint4* v, uint64_t i) {
  get_entry(a, v, 2 * i);
  fr_load(a, a);
}
__device__ inline void store_entry(uint4* v, uint64_t i, fr a) {
  fr_store(a, a);
  put_entry(v, 2 * i, a);
}
__device__ inline void words_out(uint32_t* out, const fr& a) {
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = a.v[k];
}
__device__ inline void words_in(fr& a, const uint32_t* in) {
#pragma unroll
  for (int k = 0; k < 8; k++) a.v[k] = in[k];
}

// ---------------------------------------------------------------- columns
// column `lane` of word-major rows [8][W] (neighbouring lanes, neighbouring banks)
template <int W>
__device__ inline void park(uint32_t (*rows)[W], uint32_t lane, const fr& a) {
#pragma unroll
  for (int k = 0; k < 8; k++) rows[k][lane] = a.v[k];
}
template <int W>
__device__ inline void unpark(fr& a, const uint32_t (*rows)[W], uint32_t lane) {
#pragma unroll
  for (int k = 0; k < 8; k++) a.v[k] = rows[k][lane];
}

__device__ inline void mul_add(fr& acc, const fr& x, const fr& y, const fr& c) {  // acc = x y + c
  fr t;
  fr_mul(t, x, y);
  fr_add(acc, t, c);
}

// ---------------------------------------------------------------- tree and scan over a block
// Every lane of the block calls these with its value in acc, and with rows free: no lane still reads
// or writes it. step(out, k, a, b) combines two values in step k < 8; it is inlined into the one
// copy of the loop body (the loop stays rolled: a multiplication is hundreds of instructions).
// Both end with a barrier. The tree leaves rows free. The scan leaves rows holding its results for
// scan_neighbour to read: a caller that reads them owes a barrier of its own before anything
// writes rows again (another tree or scan included); one that does not may write rows at once.
//
// Tree: step k folds the values of lanes 2 i and 2 i + 1 into lane i < 128 >> k,
// acc = step(k, lower, upper). Lane 0 ends with the fold of all 256; the other lanes' acc hold
// partial folds of no use. rows is free on return.
template <class Step>
__device__ inline void block_tree(fr& acc, uint32_t (*rows)[256], Step&& step) {
  const uint32_t tid = threadIdx.x;
  park(rows, tid, acc);
#pragma unroll 1
  for (int k = 0; k < 8; k++) {
    const uint32_t live = 128u >> k;
    __syncthreads();
    fr lo, hi;
    if (tid < live) {
      unpark(lo, rows, 2 * tid);
      unpark(hi, rows, 2 * tid + 1);
    }
    __syncthreads();
    if (tid < live) {
      step(acc, k, lo, hi);
      park(rows, tid, acc);
    }
  }
  __syncthreads();
}

// Scan, towards the higher lanes: step k combines lane l with lane l + 2^k where that lane exists,
// acc = step(k, acc, the other's). For an associative step every lane ends with the fold of the
// lanes [l, 256), nearest first; rows holds the same values, column l lane l's.
template <class Step>
__device__ inline void block_scan(fr& acc, uint32_t (*rows)[256], Step&& step) {
  const uint32_t tid = threadIdx.x;
  park(rows, tid, acc);
#pragma unroll 1
  for (int k = 0; k < 8; k++) {
    const uint32_t d = 1u << k;
    const bool live = tid + d < 256;
    __syncthreads();
    fr nb;
    if (live) unpark(nb, rows, tid + d);
    __syncthreads();
    if (live) {
      step(acc, k, acc, nb);
      park(rows, tid, acc);
    }
  }
  __syncthreads();
}
// right behind block_scan: the result of lane tid + 1, `end` for lane 255. It reads rows without a
// barrier of its own (the contract above)
__device__ inline fr scan_neighbour(const uint32_t (*rows)[256], fr end) {
  if (threadIdx.x < 255) unpark(end, rows, threadIdx.x + 1);
  return end;
}

// the sum of the 256 lanes' acc -> lane 0's acc
__device__ inline void block_sum(fr& acc, uint32_t (*rows)[256]) {
  block_tree(acc, rows, [](fr& o, int, const fr& lo, const fr& hi) { fr_add(o, lo, hi); });
}
// the sum of `count` entries of 8 words -> lane 0's acc
__device__ inline void sum_entries(fr& acc, const uint32_t* __restrict__ v, uint64_t count, uint32_t (*rows)[256]) {
  acc = fr_zero();
  for (uint64_t t = threadIdx.x; t < count; t += 256) {
    fr a;
    words_in(a, v + t * 8);
    fr_add(acc, acc, a);
  }
  block_sum(acc, rows);
}

// ---------------------------------------------------------------- powers
// x^e for e < 2^STEPS from p[k] = x^(2^k) (fr_fill_powers) and the Montgomery one: STEPS products
// in the order of k, each kept where bit k of e is set
template <int STEPS, class E>
__device__ inline fr power_from_table(const fr* p, E e, const fr& one) {
  fr acc = one;
#pragma unroll 1
  for (int k = 0; k < STEPS; k++) {
    fr nx;
    fr_mul(nx, acc, p[k]);
    if ((e >> k) & 1) acc = nx;
  }
  return acc;
}

// ---------------------------------------------------------------- tiles
template <int T>
struct Tile {
  static constexpr int S = 1 << T, M = S / 256, RUN = 2 * M + 1;  // RUN: uint4 per lane, padded
  static constexpr int SLOTS = 256 * RUN;
  static constexpr int LOG2M = T - 8;
};

// entries [blk S, (blk + 1) S) of `in` (n_in entries of 32 B; zero past the end) -> the padded tile
template <int T>
__device__ inline void stage_in(uint4* tile, const uint4* in, uint64_t blk, uint64_t n_in) {
  using G = Tile<T>;
  const uint64_t base = blk * (2 * G::S), end = 2 * n_in;
#pragma unroll
  for (int r = 0; r < 2 * G::M; r++) {
    const int i = r * 256 + (int)threadIdx.x;
    const uint64_t g = base + (uint64_t)i;
    tile[i + (i >> (G::LOG2M + 1))] = g < end ? in[g] : make_uint4(0, 0, 0, 0);
  }
}

// f(std::integral_constant<int, T>) for the tile width T = t in [MIN, MAX), MAX for any other t: the
// one place a runtime tile width picks the kernels instantiated for it
template <int MIN, int MAX, class F>
inline hipError_t with_tile(uint32_t t, F&& f) {
  if constexpr (MIN == MAX) return f(std::integral_constant<int, MAX>{});
  else return t == MIN ? f(std::integral_constant<int, MIN>{}) : with_tile<MIN + 1, MAX>(t, f);
}

}  // namespace
}  // namespace kzgpot
