// Division of a polynomial over Fr by (x - z): the evaluation and the witness polynomial of
// ark-poly-commit's KZG10::open (compute_witness_polynomial), DESIGN.md §11.
//
// For n coefficients c[0..n), lowest degree first, the suffix Horner values
//   H[j] = sum_{k >= j} c[k] z^(k-j),      H[j] = c[j] + z H[j+1]
// give p(z) = H[0] and the quotient (p(x) - p(z)) / (x - z) = sum_j H[j+1] x^j. The recurrence is
// first-order linear, so it is a scan under (A, len) o (B, len') = A + z^len B:
//
//   level 0   the n coefficients in tiles of S = 2^t; a block of 256 lanes owns a tile, a lane a run
//             of M = S / 256 consecutive coefficients
//   up        lane: Horner over its run (multiplier z); block: a tree over the 256 run sums with
//             multipliers z^M, z^2M, ... -> one sum A_b per tile. The tile sums are level 1's
//             entries: the same problem with multiplier z^S. Repeated until a level fits one tile.
//   down      from the top level: a block takes its carry H[(b+1) S] from the level above (zero at
//             the top), lane 255 adds z^M times it to its run sum, a suffix scan over the run sums
//             (8 steps, multipliers z^M .. z^128M) gives every lane its own carry, and Horner from
//             that carry writes the H of the lane's run. Levels >= 1 overwrite their sums with
//             their H (a block touches its own tile only; the carries come from the level above);
//             level 0 writes H[j] as quotient coefficient j - 1 and H[0] as the value.
//
// One stream, no grid-wide synchronisation, no look-back, no spin-wait, no cooperative launch; every
// loop's trip count is a compile-time constant. No lane does more than 2 M <= 32 Horner steps and
// 8 scan steps. Evaluate-only (no quotient) runs the up passes and the top level's down pass alone.
//
// The tree and the scan are poly_parts.hpp's block_tree and block_scan, the one place their steps
// and barriers are stated; the kernels here pass the line that combines two values.
//
// Memory (the tile and its helpers are poly_parts.hpp's, shared with eval_kernels.hip): a lane's run
// is M x 32 B at a stride of M x 32 B, so tiles are staged through LDS: every
// global load and store is one uint4 per lane at consecutive addresses, and a lane reads its run
// from LDS at a stride of 2 M + 1 uint4 (one uint4 of padding per run: an odd stride, so the 16-byte
// reads of neighbouring lanes fall into different banks). Level 0 reads 32 B per coefficient in
// the up pass, reads them again and writes 32 B in the down pass: 96 B per coefficient; the upper
// levels add 96 / S of that.
//
// The levels (entry counts, tiles, workspace offsets, which powers of z each reads) are poly_plan's
// (plans.hpp, checked on the CPU by tests/test_plan_units.py).
//
// Values are Montgomery (R = 2^256) between load and store: coefficients are 256-bit integers
// reduced on the way in (fr_load, csrc/fr.hpp), the quotient and the value leave canonical.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec.hpp"
#include "poly_parts.hpp"

namespace kzgpot {
namespace {

// y^(2^k) for this level's multiplier y = z^(S^level), k < 12, Montgomery form
struct PolyPowers {
  fr p[kPolyTileMax];
};

// the lane's run sum: sum_k c[k] z^k over its M entries. Level 0 (raw) converts each entry to
// Montgomery form and leaves it converted in the tile.
template <int T>
__device__ inline void run_sum(fr& acc, uint4* tile, bool raw, const fr& z) {
  using G = Tile<T>;
  const int s = (int)threadIdx.x * G::RUN;
#pragma unroll 1
  for (int k = G::M - 1; k >= 0; k--) {
    fr c;
    get_entry(c, tile, s + 2 * k);
    if (raw) {
      fr_load(c, c);
      put_entry(tile, s + 2 * k, c);
    }
    if (k == G::M - 1) acc = c;
    else mul_add(acc, acc, z, c);
  }
}

// ---------------------------------------------------------------- up: one sum per tile
template <int T>
__global__ void __launch_bounds__(256) k_poly_up(const uint4* __restrict__ in, uint64_t n_in, int raw,
                                                 uint32_t* __restrict__ sums, PolyPowers pw) {
  using G = Tile<T>;
  __shared__ uint4 tile[G::SLOTS];
  __shared__ uint32_t rows[8][256];
  stage_in<T>(tile, in, blockIdx.x, n_in);
  __syncthreads();
  fr acc;
  run_sum<T>(acc, tile, raw != 0, pw.p[0]);
  // a'[i] = a[2 i] + y a[2 i + 1], y = z^M, z^2M, ..: 128, 64, .. 1 live lanes
  block_tree(acc, rows, [&](fr& o, int k, const fr& lo, const fr& hi) { mul_add(o, hi, pw.p[G::LOG2M + k], lo); });
  if (threadIdx.x == 0) words_out(sums + (uint64_t)blockIdx.x * 8, acc);
}

// ---------------------------------------------------------------- down: the H of one tile
// carries: the level above's H (entry b + 1 is this tile's carry; none for the last tile).
// level0: entries are raw integers, H[j] goes out canonical as quotient coefficient j - 1; other
// levels write H[j] in Montgomery form at entry j (out may be in). out may be null (evaluate
// only). value (optional): H[0], canonical, from block 0.
template <int T>
__global__ void __launch_bounds__(256) k_poly_down(const uint4* in, uint64_t n_in, int level0, const uint32_t* carries,
                                                   uint4* out, uint32_t* __restrict__ value, PolyPowers pw) {
  using G = Tile<T>;
  __shared__ uint4 tile[G::SLOTS];
  __shared__ uint32_t rows[8][256];
  const uint32_t tid = threadIdx.x;
  const uint64_t blk = blockIdx.x;
  stage_in<T>(tile, in, blk, n_in);
  __syncthreads();
  const fr z = pw.p[0];
  fr acc, carry = fr_zero();
  run_sum<T>(acc, tile, level0 != 0, z);
  if (tid == 255 && blk + 1 < gridDim.x) {
    words_in(carry, carries + (blk + 1) * 8);
    mul_add(acc, carry, pw.p[G::LOG2M], acc);
  }
  // suffix scan: after step k lane l holds sum_{j < 2^(k+1)} y^j a[l + j], y = z^M
  block_scan(acc, rows, [&](fr& o, int k, const fr& a, const fr& nb) { mul_add(o, nb, pw.p[G::LOG2M + k], a); });
  fr h = scan_neighbour(rows, carry);  // lane 255: the tile's carry; the others: the next lane's suffix sum
  const int s = (int)tid * G::RUN;
  fr o;
#pragma unroll 1
  for (int k = G::M - 1; k >= 0; k--) {
    fr c;
    get_entry(c, tile, s + 2 * k);
    mul_add(h, h, z, c);
    o = h;
    if (level0) fr_store(o, h);
    put_entry(tile, s + 2 * k, o);
  }
  if (value && blk == 0 && tid == 0) {
    if (!level0) fr_store(o, h);
    words_out(value, o);
  }
  if (!out) return;
  __syncthreads();
  const uint64_t shift = level0 ? 1 : 0;
#pragma unroll
  for (int r = 0; r < 2 * G::M; r++) {
    const int i = r * 256 + (int)tid;
    const uint64_t e = blk * G::S + (uint64_t)(i >> 1);
    if (e >= shift && e < n_in) out[(e - shift) * 2 + (i & 1)] = tile[i + (i >> (G::LOG2M + 1))];
  }
}

// an open's last step: `words` <= 64 words behind the proof's point, unless the call was rejected
__global__ void __launch_bounds__(64) k_fr_emit(const uint32_t* __restrict__ values, uint32_t* __restrict__ out,
                                                uint32_t words, const unsigned long long* __restrict__ key) {
  if (*key != ~0ull) return;
  if (threadIdx.x < words) out[threadIdx.x] = values[threadIdx.x];
}

// The up passes, then the down passes from the top: the levels are poly_plan's (plans.hpp)
template <int T>
hipError_t launch(const PolyPlan& p, const void* d_coeffs, const fr_powers<kPolyPowers>& z_pow, void* d_quotient,
                  void* d_value, void* d_work, hipStream_t s) {
  uint8_t* w = (uint8_t*)d_work;
  auto level = [&](uint32_t k) -> void* { return k ? (void*)(w + p.level[k].off) : const_cast<void*>(d_coeffs); };
  auto powers = [&](uint32_t k) {
    PolyPowers pw;
    for (uint32_t j = 0; j < kPolyTileMax; j++) pw.p[j] = z_pow.p[p.level[k].pow0 + j];
    return pw;
  };
  auto tiles = [&](uint32_t k) { return dim3((unsigned)p.level[k].tiles); };
  for (uint32_t k = 0; k < p.top; k++)
    hipLaunchKernelGGL(k_poly_up<T>, tiles(k), dim3(256), 0, s, (const uint4*)level(k), p.level[k].cnt, k == 0 ? 1 : 0,
                       (uint32_t*)level(k + 1), powers(k));
  for (uint32_t k = p.top + 1; k-- > 0;) {
    const bool last = k == 0 || !d_quotient;  // evaluate only: the top level has the value
    hipLaunchKernelGGL(k_poly_down<T>, tiles(k), dim3(256), 0, s, (const uint4*)level(k), p.level[k].cnt, k == 0 ? 1 : 0,
                       k < p.top ? (const uint32_t*)level(k + 1) : nullptr,
                       (uint4*)(k ? (d_quotient ? level(k) : nullptr) : d_quotient), last ? (uint32_t*)d_value : nullptr,
                       powers(k));
    if (last) break;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_poly_divide(const void* d_coeffs, uint64_t n, const fr_powers<kPolyPowers>& z_pow, void* d_quotient,
                              void* d_value, uint32_t t, void* d_work, hipStream_t stream) {
  const PolyPlan p = poly_plan(n, t);
  if (!p.bytes) return hipErrorInvalidValue;
  if (n == 0) return hipMemsetAsync(d_value, 0, 32, stream);  // the zero polynomial
  return with_tile<kPolyTileMin, kPolyTileMax>(
      t, [&](auto T) { return launch<T()>(p, d_coeffs, z_pow, d_quotient, d_value, d_work, stream); });
}

hipError_t launch_fr_emit(const void* d_values, void* d_out, uint32_t words, const unsigned long long* d_key,
                          hipStream_t stream) {
  hipLaunchKernelGGL(k_fr_emit, dim3(1), dim3(64), 0, stream, (const uint32_t*)d_values, (uint32_t*)d_out, words, d_key);
  return hipGetLastError();
}

}  // namespace kzgpot
