// Variable-base multi-scalar multiplication out = sum_{i<n} [s_i] P_i in G1 or G2 — the group
// operation of ark-poly-commit's KZG10::commit (VariableBaseMSM::multi_scalar_mul over powers_of_g
// and powers_of_gamma_g), DESIGN.md §10. Scalars are 256-bit unsigned integers used as integers.
//
// Bucket method with window width c, W = ceil(256 / c) windows, NB = W 2^c buckets, built only from
// the ladders' arithmetic (jac_dbl, jac_madd, f_inv, fp_canon): no Jacobian + Jacobian addition.
//   sum_i [s_i] P_i = sum_j 2^(jc) sum_d d B[j][d],   B[j][d] = sum of the P_i whose digit j is d
//   sum_d d B[j][d] = sum_b 2^b T_(jc+b),              T_(jc+b) = sum of the B[j][d] with bit b of d set
// so the result is one double-and-add ladder over the W c "bit partials" T_k.
//
// Launch sequence (one stream, no grid-wide synchronisation, no look-back, every loop's trip count
// fixed or data-bounded; every kernel after the load returns at once if the load lowered the key):
//   k_msm_load      records -> work rows [0, n), natural order (checks as k_fft_load)
//   k_msm_count     cnt[j][d] += 1 for every finite base with digit d != 0 in window j
//   scan            off = exclusive scan of cnt, three launches: tiles, the tile sums, the add
//   k_msm_scatter   point indices into bucket order (the order inside a bucket is not fixed; a
//                   group element has one affine encoding, so the output bytes do not depend on it)
//   K levels of     k_msm_chunks + scan + k_msm_sum: every bucket's entries in chunks of at most
//                   L = kMsmChunk; one lane sums one chunk by repeated jac_madd and stores the
//                   affine partial sum; the partials of a bucket are the next level's entries.
//                   L^K >= n, so after K levels every bucket holds at most one point whatever the
//                   scalars are (a constant scalar vector puts all n points into one bucket per window)
//   bit partials    the same k_msm_sum over static index lists: W c segments of 2^(c-1) entries,
//                   again in chunks of L, until one point per segment is left
//   k_msm_final     one lane: for k = W c - 1 .. 0: double, add T_k if finite; normalise, emit
//
// L = 64: a chunk's normalisation (one inversion, about 43 mixed additions' worth) then costs at
// most 2/3 of an addition per entry of a full chunk, a lane's serial work is bounded by 64
// additions, and n = 2^26 needs K = 5 levels. A chunk of one entry is copied, not inverted.
//
// Where every launch reads and writes inside the workspace, and the list of k_msm_sum launches, is
// msm_plan's (plans.hpp, checked on the CPU by tests/test_plan_units.py).
//
// Between two additions X, Y and Z go through fp_canon (jac_canon), so every jac_madd starts from a
// canonical accumulator (or Z = 0) and a canonical base: tests/test_field_bounds_msm.py. A chunk's
// sum and the final result become affine by group_parts.hpp's canon_jac_to_affine.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "group_parts.hpp"

namespace kzgpot {
namespace {

constexpr uint32_t L = kMsmChunk;
constexpr uint32_t kNoBucket = ~0u;
constexpr uint64_t kNoSlot = ~0ull;

// ---------------------------------------------------------------- load
// One in-memory GroupAffine record (104 / 200 B: 6 LE u64 per coordinate in ark-ff Montgomery form,
// R = 2^384; an infinity byte; padding). Every coordinate < p (else 3, first failing coordinate);
// a non-zero infinity byte is the point at infinity. Out: canonical Montgomery (R = 2^392).
template <typename F>
KZG_DEV int mont_record_decode(F& x, F& y, bool& finf, const uint2* rec) {
  constexpr int NC = Geo<F>::NC;
  fp k;
  fp_set(k, FP_FROM_ARK);
  int st = 0;
#pragma unroll
  for (int c = 0; c < 2 * NC; c++) {
    words w;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const uint2 v = rec[6 * c + j];
      w[2 * j] = v.x, w[2 * j + 1] = v.y;
    }
    if (!st && words_geq_p(w)) st = 3;
    fp t;
    fp_from_words(t, w);
    fp& dst = c < NC ? comp(x, c) : comp(y, c - NC);
    fp_mul(dst, t, k);
  }
  if (st) return st;
  f_reduce_once(x);
  f_reduce_once(y);
  finf = (rec[12 * NC].x & 0xffu) != 0;
  if (finf) {
    f_zero(x);
    f_zero(y);
  }
  return 0;
}

template <typename F>
__global__ void __launch_bounds__(256) k_msm_load(const void* __restrict__ in, uint32_t* __restrict__ pool, uint64_t cap,
                                                  uint64_t n, int mont, unsigned long long* __restrict__ first_bad) {
  constexpr int NC = Geo<F>::NC;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  F x, y;
  bool finf = false;
  const int st = mont ? mont_record_decode(x, y, finf, (const uint2*)in + i * (12 * NC + 1))
                      : ark_record_decode(x, y, finf, (const uint4*)in + i * (6 * NC));
  report(i, st, first_bad, nullptr);
  if (st) return;
  work_store_point(pool, cap, i, x, y, finf);
}

// ---------------------------------------------------------------- digits, count, scatter
// digit j (c bits from bit j c) of the 256-bit scalar at s[0..8); bits past 255 are zero
KZG_DEV uint32_t msm_digit(const uint32_t* s, uint32_t j, uint32_t c) {
  const uint32_t bit = j * c, w = bit >> 5, sh = bit & 31;
  uint64_t v = w < 8 ? s[w] : 0;
  if (w + 1 < 8) v |= (uint64_t)s[w + 1] << 32;
  return (uint32_t)(v >> sh) & ((1u << c) - 1);
}
// the bucket of (point i, window j): none for an infinite base, a zero digit or i >= n
KZG_DEV uint32_t msm_bucket(const uint32_t* scalars, const uint32_t* inf, uint64_t i, uint64_t n, uint32_t j, uint32_t c) {
  if (i >= n || inf[i]) return kNoBucket;
  const uint32_t d = msm_digit(scalars + i * 8, j, c);
  return d ? (j << c) | d : kNoBucket;
}

// One lane per point, W windows each. When a whole wave targets one bucket (equal scalars) its
// first lane issues one atomic for all 64: a constant scalar vector would otherwise serialise n
// atomics per window on one address.
__global__ void __launch_bounds__(256) k_msm_count(const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ inf,
                                                   uint64_t n, uint32_t c, uint32_t nwin, uint32_t* __restrict__ cnt,
                                                   const unsigned long long* __restrict__ key) {
  if (rejected(key)) return;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lanes = (uint32_t)__popcll(__ballot(1));  // no lane has left: the whole wave, counted out here
#pragma unroll 1
  for (uint32_t j = 0; j < nwin; j++) {
    const uint32_t b = msm_bucket(scalars, inf, i, n, j, c);
    const uint32_t lead = __builtin_amdgcn_readfirstlane(b);
    if (__all(b == lead)) {
      if (lead != kNoBucket && __lane_id() == 0) atomicAdd(cnt + lead, lanes);
    } else if (b != kNoBucket) {
      atomicAdd(cnt + b, 1u);
    }
  }
}

// idx[off[b] + (a slot below cnt[b])] = i; cnt counts down to zero
__global__ void __launch_bounds__(256) k_msm_scatter(const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ inf,
                                                     uint64_t n, uint32_t c, uint32_t nwin, uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ off, uint32_t* __restrict__ idx,
                                                     const unsigned long long* __restrict__ key) {
  if (rejected(key)) return;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lanes = (uint32_t)__popcll(__ballot(1));  // as k_msm_count
#pragma unroll 1
  for (uint32_t j = 0; j < nwin; j++) {
    const uint32_t b = msm_bucket(scalars, inf, i, n, j, c);
    const uint32_t lead = __builtin_amdgcn_readfirstlane(b);
    if (__all(b == lead)) {
      if (lead == kNoBucket) continue;
      uint32_t old = 0;
      if (__lane_id() == 0) old = atomicSub(cnt + lead, lanes);  // old >= lanes: this wave's own share is in cnt
      old = __builtin_amdgcn_readfirstlane(old);
      idx[off[lead] + old - 1 - __lane_id()] = (uint32_t)i;
    } else if (b != kNoBucket) {
      idx[off[b] + atomicSub(cnt + b, 1u) - 1] = (uint32_t)i;
    }
  }
}

// ---------------------------------------------------------------- exclusive scan, three launches
// tile t: off[i] = sum of in[tile start .. i) for its entries i < nb, sums[t] = the tile's total
// (in may be off: every lane reads its entries before any lane writes)
__global__ void __launch_bounds__(256) k_msm_scan_tiles(const uint32_t* in, uint32_t* off, uint32_t* __restrict__ sums,
                                                        uint32_t nb, const unsigned long long* __restrict__ key) {
  __shared__ uint32_t sh[256];
  if (rejected(key)) return;
  const uint32_t tid = threadIdx.x, base = blockIdx.x * kScanTile + tid * kScanItems;
  uint32_t v[kScanItems], run = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; k++) {
    const uint32_t x = base + k < nb ? in[base + k] : 0;
    v[k] = run;
    run += x;
  }
  sh[tid] = run;
  __syncthreads();
#pragma unroll 1
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t t = tid >= d ? sh[tid - d] : 0;
    __syncthreads();
    sh[tid] += t;
    __syncthreads();
  }
  const uint32_t excl = sh[tid] - run;
#pragma unroll
  for (int k = 0; k < kScanItems; k++)
    if (base + k < nb) off[base + k] = excl + v[k];
  if (tid == 255) sums[blockIdx.x] = sh[255];
}
// off[i] += (scanned) sums[tile of i]; off[nb] = the total, sums[ntiles]
__global__ void __launch_bounds__(256) k_msm_scan_add(uint32_t* __restrict__ off, const uint32_t* __restrict__ sums,
                                                      uint32_t nb, uint32_t ntiles,
                                                      const unsigned long long* __restrict__ key) {
  if (rejected(key)) return;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < nb) off[i] += sums[i / kScanTile];
  if (i == 0) off[nb] = sums[ntiles];
}
// the next level's counts: bucket b's entries in chunks of L
__global__ void __launch_bounds__(256) k_msm_chunks(const uint32_t* __restrict__ off, uint32_t* __restrict__ cnt,
                                                    uint32_t nb, const unsigned long long* __restrict__ key) {
  if (rejected(key)) return;
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b < nb) cnt[b] = (off[b + 1] - off[b] + L - 1) / L;
}

// ---------------------------------------------------------------- segmented sum to affine
// Lane q sums one chunk (at most L entries) of one segment and stores the affine sum at pool slot
// out_base + q.
//   mode 0  buckets, level 0: segment b = entries [off_in[b], off_in[b+1]) of idx (work-row slots of bases)
//   mode 1  buckets, level k: the same over the previous level's partials, entry e at in_base + e
//           (both: chunk q belongs to the bucket b with off_out[b] <= q < off_out[b+1])
//   mode 2  bit partials, level 0: segment s = (window j = s / c, bit b = s % c), entry e = the
//           bucket (j, d) with d = e's bits with a one inserted at bit b; its point is at
//           in_base + off_in[(j, d)] if the bucket is not empty
//   mode 3  bit partials, level k: segment s = entries [s seg_len, (s + 1) seg_len) at in_base
// (modes 2, 3: seg_chunks chunks per segment). Infinite entries are skipped.
struct SumArgs {
  const uint32_t* idx;
  const uint32_t* off_in;
  const uint32_t* off_out;
  uint64_t in_base, out_base;
  uint32_t mode, nb, c, nseg, seg_len, seg_chunks;
};

template <typename F>
__global__ void __launch_bounds__(Geo<F>::BLOCK) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_msm_sum(uint32_t* pool, uint64_t cap, SumArgs a, const unsigned long long* __restrict__ key) {
  constexpr int BLOCK = Geo<F>::BLOCK, INF = Geo<F>::INF_ROW;
  if (rejected(key)) return;
  const uint64_t q = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  uint32_t start, end, seg = 0;
  if (a.mode < 2) {
    if (q >= a.off_out[a.nb]) return;
    uint32_t lo = 0, hi = a.nb;  // off_out[lo] <= q < off_out[hi]
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.off_out[mid] <= q) lo = mid;
      else hi = mid;
    }
    start = a.off_in[lo] + ((uint32_t)q - a.off_out[lo]) * L;
    end = min(start + L, a.off_in[lo + 1]);
  } else {
    if (q >= (uint64_t)a.nseg * a.seg_chunks) return;
    seg = (uint32_t)(q / a.seg_chunks);
    start = (uint32_t)(q % a.seg_chunks) * L;
    end = min(start + L, a.seg_len);
  }
  const uint32_t* rd = opaque((const uint32_t*)pool);
  auto slot_of = [&](uint32_t e) -> uint64_t {
    uint64_t s;
    if (a.mode == 0) {
      s = a.idx[e];
    } else if (a.mode == 1) {
      s = a.in_base + e;
    } else if (a.mode == 2) {
      const uint32_t j = seg / a.c, b = seg % a.c;
      const uint32_t d = ((e >> b) << (b + 1)) | (1u << b) | (e & ((1u << b) - 1));
      const uint32_t bk = (j << a.c) | d, o = a.off_in[bk];
      if (a.off_in[bk + 1] == o) return kNoSlot;
      s = a.in_base + o;
    } else {
      s = a.in_base + (uint64_t)seg * a.seg_len + e;
    }
    return rd[(uint64_t)INF * cap + s] ? kNoSlot : s;
  };

  jac<F> acc;
  jac_set_infinity(acc);
  int adds = 0;
#pragma unroll 1
  for (uint32_t e = start; e < end; e++) {
    const uint64_t s = slot_of(e);
    if (s == kNoSlot) continue;
    jac_madd(acc, [&](F& x, F& y) { work_load_xy(x, y, opaque(rd), cap, s); });
    jac_canon(acc);
    adds++;
  }
  const bool inf = f_is_zero(acc.z);
  F x = acc.x, y = acc.y;
  if (adds > 1) canon_jac_to_affine(x, y, acc, inf);  // one entry: Z = 1 and (X, Y) is the entry
  work_store_point(pool, cap, a.out_base + q, x, y, inf);
}

// ---------------------------------------------------------------- final ladder
// One lane: acc = sum_k 2^k T_k by double-and-add from the top bit (the ladders' proven
// "double, then optionally add a canonical base" step), T_k at slot in_base + k; one record out.
template <typename F>
__global__ void __launch_bounds__(64) k_msm_final(const uint32_t* __restrict__ pool, uint64_t cap, uint64_t in_base,
                                                  int nbits, uint4* __restrict__ out,
                                                  const unsigned long long* __restrict__ key) {
  constexpr int INF = Geo<F>::INF_ROW;
  if (rejected(key) || threadIdx.x || blockIdx.x) return;
  jac<F> acc;
  jac_set_infinity(acc);
#pragma unroll 1
  for (int k = nbits - 1; k >= 0; k--) {
    jac_dbl(acc);
    const uint64_t s = in_base + (uint64_t)k;
    if (opaque(pool)[(uint64_t)INF * cap + s]) continue;
    jac_madd(acc, [&](F& x, F& y) { work_load_xy(x, y, opaque(pool), cap, s); });
  }
  if (f_is_zero(acc.z)) {
    emit_infinity<F>(out, false);
    return;
  }
  jac_canon(acc);
  F x, y;
  canon_jac_to_affine(x, y, acc, false);
  emit_point(out, x, y, false);
}

// ---------------------------------------------------------------- launch
// The fixed prologue, then the plan's steps (plans.hpp: every region, base and lane count is the plan's)
template <typename F>
hipError_t launch(const MsmPlan& p, const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, bool mont,
                  void* d_work, unsigned long long* key, hipStream_t s) {
  constexpr int BLOCK = Geo<F>::BLOCK;
  uint8_t* w = (uint8_t*)d_work;
  uint32_t* cnt = (uint32_t*)(w + p.cnt);
  uint32_t* sums = (uint32_t*)(w + p.sums);
  uint32_t* idx = (uint32_t*)(w + p.idx);
  uint32_t* pool = (uint32_t*)(w + p.pool);
  const uint32_t* inf = pool + (uint64_t)Geo<F>::INF_ROW * p.cap;
  const uint32_t* scalars = (const uint32_t*)d_scalars;
  const dim3 b256(256);
  auto offsets = [&](uint64_t at) { return at == kMsmNoOffsets ? nullptr : (uint32_t*)(w + at); };
  auto scan = [&](uint32_t* off) {  // off = exclusive scan of cnt, off[nb] = total
    hipLaunchKernelGGL(k_msm_scan_tiles, dim3(p.ntiles), b256, 0, s, cnt, off, sums, p.nb, key);
    hipLaunchKernelGGL(k_msm_scan_tiles, dim3(1), b256, 0, s, sums, sums, sums + p.ntiles, p.ntiles, key);
    hipLaunchKernelGGL(k_msm_scan_add, dim3(grid_for(p.nb, 256)), b256, 0, s, off, sums, p.nb, p.ntiles, key);
  };
  if (hipError_t e = hipMemsetAsync(cnt, 0, (size_t)p.nb * 4, s)) return e;
  hipLaunchKernelGGL(k_msm_load<F>, dim3(grid_for(n, 256)), b256, 0, s, d_bases, pool, p.cap, n, mont ? 1 : 0, key);
  hipLaunchKernelGGL(k_msm_count, dim3(grid_for(n, 256)), b256, 0, s, scalars, inf, n, p.c, p.nwin, cnt, key);
  scan(offsets(p.off_a));
  hipLaunchKernelGGL(k_msm_scatter, dim3(grid_for(n, 256)), b256, 0, s, scalars, inf, n, p.c, p.nwin, cnt,
                     offsets(p.off_a), idx, key);
  for (uint32_t k = 0; k < p.nsteps; k++) {
    const MsmStep& st = p.step[k];
    const bool buckets = st.mode < 2;
    uint32_t *off_in = offsets(st.off_in), *off_out = offsets(st.off_out);
    if (buckets) {
      hipLaunchKernelGGL(k_msm_chunks, dim3(grid_for(p.nb, 256)), b256, 0, s, off_in, cnt, p.nb, key);
      scan(off_out);
    }
    const SumArgs a = {buckets ? idx : nullptr, off_in, off_out, st.in_base, st.out_base, st.mode, p.nb, p.c,
                       st.nseg, st.seg_len, st.seg_chunks};
    hipLaunchKernelGGL(k_msm_sum<F>, dim3(grid_for(st.lanes, BLOCK)), dim3(BLOCK), 0, s, pool, p.cap, a, key);
  }
  hipLaunchKernelGGL(k_msm_final<F>, dim3(1), dim3(64), 0, s, pool, p.cap, p.final_base, (int)p.nseg, (uint4*)d_out, key);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_msm(bool g2, const void* d_bases, const void* d_scalars, uint64_t n, void* d_out, bool mont,
                      uint32_t c, void* d_work, unsigned long long* d_key, hipStream_t stream) {
  const MsmPlan p = msm_plan(g2, n, c);
  if (!p.ok) return hipErrorInvalidValue;
  return g2 ? launch<fp2>(p, d_bases, d_scalars, n, d_out, mont, d_work, d_key, stream)
            : launch<fp>(p, d_bases, d_scalars, n, d_out, mont, d_work, d_key, stream);
}

}  // namespace kzgpot
