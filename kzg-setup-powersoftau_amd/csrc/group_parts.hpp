// Device functions that the group kernels (fft_kernels.hip: the group FFT; msm_kernels.hip: the
// multi-scalar multiplication) share, each stated once: the limb-major work rows, the ark record
// decode with the loaders' checks, the canonical-value helpers for both fields, the Jacobian ->
// affine tail (jac_to_affine: the one statement of "zero test, canonicalise, invert Z, scale") and
// the record emit. All force-inlined.
//
// Work rows: limb-major rows of `m` words, row k holding word k of every point (a wave's accesses
// to one row are contiguous wherever its points are): x (NW rows), y (NW rows), then one row that
// is 1 for the point at infinity and 0 otherwise (NW = 14 for G1, 28 for G2). Coordinates are
// canonical Montgomery values (< p), so every consumer starts from the ladders' proven base bounds
// (tests/test_field_bounds_lagrange.py, tests/test_field_bounds_msm.py).
#pragma once
#include "codec_parts.hpp"

namespace kzgpot {

template <typename F>
struct Geo {
  static constexpr int NW = sizeof(F) / 4;  // words per field element: 14 (Fp), 28 (Fp2)
  static constexpr int NC = NW / NL;        // Fp coordinates per field element
  static constexpr int INF_ROW = 2 * NW;    // work-buffer row of the infinity mark
  static constexpr int ROWS = 2 * NW + 1;   // rows of a point
  // butterflies per block: 2 NW LDS rows per lane = 28 KB either way (4 blocks = 8 waves per CU)
  static constexpr int BLOCK = NC == 1 ? 256 : 128;
};
static_assert(Geo<fp>::ROWS == kWorkRowsG1 && Geo<fp2>::ROWS == kWorkRowsG2, "the plans' row counts (plans.hpp)");
static_assert(Geo<fp>::INF_ROW == kWorkRowsG1 - 1 && Geo<fp2>::INF_ROW == kWorkRowsG2 - 1, "the last row marks infinity");

// ---------------------------------------------------------------- field helpers, both fields
KZG_DEV fp& comp(fp& a, int) { return a; }
KZG_DEV fp& comp(fp2& a, int c) { return c ? a.c1 : a.c0; }
KZG_DEV const fp& comp(const fp& a, int) { return a; }
KZG_DEV const fp& comp(const fp2& a, int c) { return c ? a.c1 : a.c0; }

// any ladder or mixed-addition output (limbs < 2^32 - 16, value < 256 p) -> canonical
template <typename F>
KZG_DEV void f_canon(F& a) {
#pragma unroll
  for (int c = 0; c < Geo<F>::NC; c++) fp_canon(comp(a, c), comp(a, c));
}
// a product of canonical values (normalized, value < 2 p) -> canonical
template <typename F>
KZG_DEV void f_reduce_once(F& a) {
#pragma unroll
  for (int c = 0; c < Geo<F>::NC; c++) fp_reduce_once(comp(a, c), comp(a, c));
}
// canonical -> canonical negation
template <typename F>
KZG_DEV void f_neg_canon(F& a) {
#pragma unroll
  for (int c = 0; c < Geo<F>::NC; c++) fp_neg_canon(comp(a, c), comp(a, c));
}
template <typename F>
KZG_DEV void f_zero(F& a) {
#pragma unroll
  for (int c = 0; c < Geo<F>::NC; c++) fp_zero(comp(a, c));
}
template <typename F>
KZG_DEV void f_select(F& r, bool c, const F& a, const F& b) {
#pragma unroll
  for (int k = 0; k < Geo<F>::NC; k++) fp_select(comp(r, k), c, comp(a, k), comp(b, k));
}

// ---------------------------------------------------------------- work buffer and LDS rows
template <typename F>
KZG_DEV void work_load(F& a, const uint32_t* work, uint64_t m, int row, uint64_t idx) {
  uint32_t* d = (uint32_t*)&a;
#pragma unroll
  for (int k = 0; k < Geo<F>::NW; k++) d[k] = work[(uint64_t)(row + k) * m + idx];
}
template <typename F>
KZG_DEV void work_load_xy(F& x, F& y, const uint32_t* work, uint64_t m, uint64_t idx) {
  work_load(x, work, m, 0, idx);
  work_load(y, work, m, Geo<F>::NW, idx);
}
template <typename F>
KZG_DEV void work_store(uint32_t* work, uint64_t m, int row, uint64_t idx, const F& a) {
  const uint32_t* s = (const uint32_t*)&a;
#pragma unroll
  for (int k = 0; k < Geo<F>::NW; k++) work[(uint64_t)(row + k) * m + idx] = s[k];
}
template <typename F>
KZG_DEV void work_store_point(uint32_t* work, uint64_t m, uint64_t idx, const F& x, const F& y, bool inf) {
  work_store(work, m, 0, idx, x);
  work_store(work, m, Geo<F>::NW, idx, y);
  work[(uint64_t)Geo<F>::INF_ROW * m + idx] = inf ? 1u : 0u;
}

// a lane's column of a __shared__ uint32_t [rows][BLOCK] array (as codec_parts.hpp's lds_rows)
template <typename F, int BLOCK>
KZG_DEV void park(uint32_t (*rows)[BLOCK], const F& a) {
  const uint32_t* s = (const uint32_t*)&a;
#pragma unroll
  for (int k = 0; k < Geo<F>::NW; k++) rows[k][threadIdx.x] = s[k];
}
template <typename F, int BLOCK>
KZG_DEV void unpark(F& a, const uint32_t (*rows)[BLOCK], uint32_t lane) {
  uint32_t* d = (uint32_t*)&a;
#pragma unroll
  for (int k = 0; k < Geo<F>::NW; k++) d[k] = rows[k][lane];
}

KZG_DEV bool rejected(const unsigned long long* key) { return *key != ~0ull; }

// ---------------------------------------------------------------- ark record -> work-row values
// One ark-uncompressed record (96 / 192 B at rec). Checks as k_load_direct (load_kernels.hip), in
// ark's read order: every coordinate < p (3), both SWFlags set (6, parsed before the last
// coordinate's range check). Returns the status; on 0, (x, y) canonical Montgomery and finf the
// infinity flag (a flagged infinity keeps no coordinates).
template <typename F>
KZG_DEV int ark_record_decode(F& x, F& y, bool& finf, const uint4* rec) {
  constexpr int NC = Geo<F>::NC;
  words w[2 * NC];
#pragma unroll
  for (int c = 0; c < 2 * NC; c++) load_le(w[c], rec + 3 * c);
  bool both;
  finf = ark_sw_flags(w[2 * NC - 1][11], both);
  int st = 0;
#pragma unroll
  for (int c = 0; c < 2 * NC - 1; c++)
    if (!st && words_geq_p(w[c])) st = 3;
  if (!st && both) st = 6;
  if (!st && words_geq_p(w[2 * NC - 1])) st = 3;
  if (st) return st;
  // written out: as a loop the four Fp2 conversions are past the unroller's size limit, and a loop
  // left rolled indexes w dynamically, which puts it into scratch
  words_to_mont(comp(x, 0), w[0]);
  words_to_mont(comp(y, 0), w[NC]);
  if constexpr (NC == 2) {
    words_to_mont(x.c1, w[1]);
    words_to_mont(y.c1, w[3]);
  }
  f_reduce_once(x);
  f_reduce_once(y);
  if (finf) {
    f_zero(x);
    f_zero(y);
  }
  return 0;
}

// ---------------------------------------------------------------- Jacobian -> affine
// x = X zi^2, y = Y zi^3 for canonical X, Y, zi: canonical out (zero if inf)
template <typename F>
KZG_DEV void scale_to_affine(F& x, F& y, const F& X, const F& Y, const F& zi, bool inf) {
  F z2;
  f_sqr(z2, zi);
  f_mul(x, X, z2);
  f_mul(z2, z2, zi);
  f_mul(y, Y, z2);
  f_reduce_once(x);
  f_reduce_once(y);
  if (inf) {
    f_zero(x);
    f_zero(y);
  }
}

template <typename F>
KZG_DEV void jac_set_infinity(jac<F>& acc) {  // X = Y = Z = 0: jac_dbl keeps it, jac_madd replaces it by its operand
  f_zero(acc.x);
  f_zero(acc.y);
  f_zero(acc.z);
}
template <typename F>
KZG_DEV void jac_canon(jac<F>& acc) {
  f_canon(acc.x);
  f_canon(acc.y);
  f_canon(acc.z);
}
// a canonical accumulator and its infinity flag -> canonical affine (x, y), zero if inf: Z (1 for
// an infinite one) inverted once. With a constant inf = false the selects fold away.
template <typename F>
KZG_DEV void canon_jac_to_affine(F& x, F& y, jac<F>& acc, bool inf) {
  F one, zi;
  f_one(one);
  f_select(acc.z, inf, one, acc.z);
  f_inv(zi, acc.z);
  f_reduce_once(zi);
  scale_to_affine(x, y, acc.x, acc.y, zi, inf);
}
// an accumulator as a ladder or a mixed addition left it -> canonical affine; returns whether it
// is the point at infinity (Z = 0, tested before Z is canonicalised)
template <typename F>
KZG_DEV bool jac_to_affine(F& x, F& y, jac<F>& acc) {
  const bool inf = f_is_zero(acc.z);
  jac_canon(acc);
  canon_jac_to_affine(x, y, acc, inf);
  return inf;
}

// ---------------------------------------------------------------- emit
KZG_DEV void store_canon_be(uint4* dst, const fp& c) {  // canonical -> 48 big-endian bytes
  words w, e;
  fp_to_words(w, c);
#pragma unroll
  for (int k = 0; k < 12; k++) e[k] = bswap32(w[11 - k]);
  store_words(dst, e);
}

// a finite point's record: ark LE (x, y; Fp2 c0 first) or pairing BE (x, y; Fp2 c1 first — the
// per-coordinate byte reversal of the ark record, A6); x, y Montgomery, normalized
template <typename F>
KZG_DEV void emit_point(uint4* dst, const F& x, const F& y, bool pairing) {
  constexpr int NC = Geo<F>::NC;
#pragma unroll
  for (int c = 0; c < 2 * NC; c++) {
    const F& v = c < NC ? x : y;
    fp canon;
    fp_from_mont(canon, comp(v, c % NC));
    if (pairing) store_canon_be(dst + 3 * (c < NC ? NC - 1 - c : 3 * NC - 1 - c), canon);
    else store_canon(dst + 3 * c, canon);
  }
}
// the point at infinity: ark GroupAffine::zero() = (0, 1, infinity flag); pairing into_uncompressed
// = 0x40 then zeros
template <typename F>
KZG_DEV void emit_infinity(uint4* dst, bool pairing) {
  constexpr int NC = Geo<F>::NC;
  if (!pairing) {
    emit_no_point<NC>(dst, true, false);
    return;
  }
  store_zero(dst, 6 * NC);
  dst[0] = make_uint4(0x40u, 0, 0, 0);
}

}  // namespace kzgpot
