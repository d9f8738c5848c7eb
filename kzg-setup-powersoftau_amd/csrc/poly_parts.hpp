// The padded-run tile that the kernels over Fr vectors share (poly_kernels.hip: the polynomial
// division; eval_kernels.hip: the batch inversion and the division in evaluation form). A block of
// 256 lanes owns a tile of S = 2^T entries of 32 B, a lane a run of M = S / 256 consecutive entries.
// Global loads and stores are one uint4 per lane at consecutive addresses; in LDS a run takes
// 2 M + 1 uint4 (one of padding: an odd stride, so the 16-byte accesses of neighbouring lanes fall
// into different banks). `rows` is a lane's column of one value per lane, word-major.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fr.hpp"

namespace kzgpot {
namespace {

template <int T>
struct Tile {
  static constexpr int S = 1 << T, M = S / 256, RUN = 2 * M + 1;  // RUN: uint4 per lane, padded
  static constexpr int SLOTS = 256 * RUN;
  static constexpr int LOG2M = T - 8;
};

__device__ inline void tile_get(fr& a, const uint4* tile, int slot) {
  const uint4 lo = tile[slot], hi = tile[slot + 1];
  a.v[0] = lo.x, a.v[1] = lo.y, a.v[2] = lo.z, a.v[3] = lo.w;
  a.v[4] = hi.x, a.v[5] = hi.y, a.v[6] = hi.z, a.v[7] = hi.w;
}
__device__ inline void tile_put(uint4* tile, int slot, const fr& a) {
  tile[slot] = make_uint4(a.v[0], a.v[1], a.v[2], a.v[3]);
  tile[slot + 1] = make_uint4(a.v[4], a.v[5], a.v[6], a.v[7]);
}
// a lane's column of the 256 run sums (word-major: neighbouring lanes, neighbouring banks)
__device__ inline void park(uint32_t (*rows)[256], uint32_t lane, const fr& a) {
#pragma unroll
  for (int k = 0; k < 8; k++) rows[k][lane] = a.v[k];
}
__device__ inline void unpark(fr& a, const uint32_t (*rows)[256], uint32_t lane) {
#pragma unroll
  for (int k = 0; k < 8; k++) a.v[k] = rows[k][lane];
}
__device__ inline void mul_add(fr& acc, const fr& x, const fr& y, const fr& c) {  // acc = x y + c
  fr t;
  fr_mul(t, x, y);
  fr_add(acc, t, c);
}

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

// ---------------------------------------------------------------- sums over a block, entries in HBM
// (eval_kernels.hip: the division in evaluation form; verify_kernels.hip: the check's Fr pass)
__device__ inline fr fr_zero() { return fr{{0, 0, 0, 0, 0, 0, 0, 0}}; }

// the sum of the 256 lanes' acc -> lane 0's acc (rows is free on entry and on return)
__device__ inline void block_sum(fr& acc, uint32_t (*rows)[256]) {
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
      fr_add(acc, lo, hi);
      park(rows, tid, acc);
    }
  }
  __syncthreads();
}

__device__ inline void load_entry(fr& a, const uint4* v, uint64_t i) {  // any 256-bit integer -> Montgomery
  const uint4 lo = v[2 * i], hi = v[2 * i + 1];
  a = fr{{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}};
  fr_load(a, a);
}
__device__ inline void words_out(uint32_t* out, const fr& a) {
#pragma unroll
  for (int k = 0; k < 8; k++) out[k] = a.v[k];
}
__device__ inline void words_in(fr& a, const uint32_t* in) {
#pragma unroll
  for (int k = 0; k < 8; k++) a.v[k] = in[k];
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

}  // namespace
}  // namespace kzgpot
