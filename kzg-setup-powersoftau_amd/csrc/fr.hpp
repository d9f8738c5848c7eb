// BLS12-381 scalar field Fr (the group order r) for the group FFT's twiddle factors: 8 x 32-bit
// little-endian words, Montgomery form with R = 2^256, one CIOS multiply shared by the host
// (domain root, the powers w^(2^k), m^-1: phase2.hip) and the device (k_fft_twiddles builds w^j from
// those powers, fft_kernels.hip). Nothing there is hot: ~31 multiplies per twiddle against the 254
// point doublings the twiddle then drives. The polynomial division of KZG10 open
// (poly_kernels.hip, open.hip) adds the rest of the field: add, sub, load and store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bls12_381_consts.hpp"

namespace kzgpot {

struct fr {
  uint32_t v[8];
};

// r = 1 (mod 2^32), so -r^-1 mod 2^32 is all ones
constexpr uint32_t FR_NINV = 0xffffffffu;
static_assert(FR_R[0] == 1u, "FR_NINV assumes r = 1 mod 2^32");

// a >= r ? a - r : a, for a < 2r given as 8 words plus a carry word
__host__ __device__ inline void fr_cond_sub(fr& out, const uint32_t (&t)[9]) {
  uint32_t d[8];
  int64_t br = 0;
  for (int i = 0; i < 8; i++) {
    const int64_t s = (int64_t)t[i] - (int64_t)FR_R[i] + br;
    d[i] = (uint32_t)s;
    br = s >> 32;  // 0 or -1
  }
  const bool ge = (int64_t)t[8] + br >= 0;
  for (int i = 0; i < 8; i++) out.v[i] = ge ? d[i] : t[i];
}

// out = a b R^-1 mod r for a, b < r (CIOS); out < r
__host__ __device__ inline void fr_mul(fr& out, const fr& a, const fr& b) {
  uint32_t t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
    for (int j = 0; j < 8; j++) {
      const uint64_t s = (uint64_t)a.v[j] * b.v[i] + t[j] + c;
      t[j] = (uint32_t)s;
      c = s >> 32;
    }
    uint64_t s = (uint64_t)t[8] + c;
    t[8] = (uint32_t)s;
    t[9] = (uint32_t)(s >> 32);
    const uint32_t m = t[0] * FR_NINV;
    c = ((uint64_t)m * FR_R[0] + t[0]) >> 32;
    for (int j = 1; j < 8; j++) {
      s = (uint64_t)m * FR_R[j] + t[j] + c;
      t[j - 1] = (uint32_t)s;
      c = s >> 32;
    }
    s = (uint64_t)t[8] + c;
    t[7] = (uint32_t)s;
    t[8] = t[9] + (uint32_t)(s >> 32);
  }
  const uint32_t r9[9] = {t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]};
  fr_cond_sub(out, r9);
}

// Montgomery -> canonical: a * 1
__host__ __device__ inline void fr_from_mont(fr& out, const fr& a) {
  fr one = {{1, 0, 0, 0, 0, 0, 0, 0}};
  fr_mul(out, a, one);
}

// ---------------------------------------------------------------- polynomial arithmetic (poly_kernels.hip, open.hip)
// out = a + b mod r for a, b < r
__host__ __device__ inline void fr_add(fr& out, const fr& a, const fr& b) {
  uint32_t t[9];
  uint64_t c = 0;
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a.v[i] + b.v[i];
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  t[8] = (uint32_t)c;
  fr_cond_sub(out, t);
}

// out = a - b mod r for a, b < r
__host__ __device__ inline void fr_sub(fr& out, const fr& a, const fr& b) {
  uint32_t d[8];
  int64_t br = 0;
  for (int i = 0; i < 8; i++) {
    const int64_t s = (int64_t)a.v[i] - (int64_t)b.v[i] + br;
    d[i] = (uint32_t)s;
    br = s >> 32;  // 0 or -1
  }
  const uint32_t mask = (uint32_t)br;  // all ones: a < b, add r back
  uint64_t c = 0;
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)d[i] + (FR_R[i] & mask);
    out.v[i] = (uint32_t)c;
    c >>= 32;
  }
}

// R = 2^256 mod r (the Montgomery one) and R^2 mod r, by 256 and 512 doublings at compile time
struct fr_radix {
  uint32_t one[8], r2[8];
};
constexpr fr_radix fr_make_radix() {
  fr_radix k = {};
  uint32_t x[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 512; i++) {  // x = 2^(i + 1) mod r
    uint32_t t[9] = {}, d[8] = {}, c = 0;
    for (int j = 0; j < 8; j++) {
      t[j] = (x[j] << 1) | c;
      c = x[j] >> 31;
    }
    t[8] = c;
    int64_t br = 0;
    for (int j = 0; j < 8; j++) {
      const int64_t s = (int64_t)t[j] - (int64_t)FR_R[j] + br;
      d[j] = (uint32_t)s;
      br = s < 0 ? -1 : 0;
    }
    const bool ge = (int64_t)t[8] + br >= 0;
    for (int j = 0; j < 8; j++) x[j] = ge ? d[j] : t[j];
    if (i == 255)
      for (int j = 0; j < 8; j++) k.one[j] = x[j];
  }
  for (int j = 0; j < 8; j++) k.r2[j] = x[j];
  return k;
}
constexpr fr_radix FR_RADIX = fr_make_radix();

// Load: any 256-bit integer a (8 LE words; 2^256 - 1 is legal and means its residue) -> the
// Montgomery form of a mod r, as one multiplication by R^2 mod r. Bound: CIOS returns
// (a b + m r) / R for some m < R before its conditional subtraction; with a < R = 2^256 and
// b = R^2 mod r < r that is below a b / R + r < b + r < 2 r, which is what fr_cond_sub takes, so the
// result is reduced although a itself may be as large as 2.2 r. Inside the loop the running value
// stays below R + 2 r < 2^258 (each round adds at most (R + r) 2^32 before its shift by 2^32): it
// fits the nine words and the transient tenth.
__host__ __device__ inline void fr_load(fr& out, const fr& a) {
  fr r2;
  for (int i = 0; i < 8; i++) r2.v[i] = FR_RADIX.r2[i];
  fr_mul(out, a, r2);
}
// Store: Montgomery form -> the canonical value below r (8 LE words: 32 little-endian bytes)
__host__ __device__ inline void fr_store(fr& out, const fr& a) { fr_from_mont(out, a); }

}  // namespace kzgpot
