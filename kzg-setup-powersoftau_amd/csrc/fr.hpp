// BLS12-381 scalar field Fr (the group order r), stated once for the host and the device: 8 x 32-bit
// little-endian words, Montgomery form with R = 2^256, one CIOS multiply. The ABI units start from
// the host helpers at the end (phase2.hip: the domain root, the powers w^(+-2^k), 1/m; open.hip: the
// powers z^(2^k)); the kernels use the arithmetic (fft_kernels.hip: k_fft_twiddles builds w^j from
// those powers; poly_kernels.hip: the polynomial division of KZG10 open; ntt_kernels.hip: the NTT's
// butterflies, the one place where these multiplies are the hot path). Elsewhere nothing here is
// hot: ~31 multiplies per twiddle against the 254 point doublings the twiddle then drives.
//
// Plain C++17 unless the compiler is hipcc, so a host program can include this file alone
// (tests/host_units/fr_units.cpp, built by g++ with and without sanitizers).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KZG_HD __host__ __device__ inline
#else
#define KZG_HD inline
#endif
#include <stdint.h>

#include "bls12_381_consts.hpp"

namespace kzgpot {

// An element in Montgomery form, or (where a comment says so) a plain 256-bit integer
struct fr {
  uint32_t v[8];
};

// r = 1 (mod 2^32), so -r^-1 mod 2^32 is all ones
constexpr uint32_t FR_NINV = 0xffffffffu;
static_assert(FR_R[0] == 1u, "FR_NINV assumes r = 1 mod 2^32");

// a >= r ? a - r : a, for a < 2r given as 8 words plus a carry word
KZG_HD constexpr void fr_cond_sub(fr& out, const uint32_t (&t)[9]) {
  uint32_t d[8] = {};
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
KZG_HD void fr_mul(fr& out, const fr& a, const fr& b) {
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

// out = a + b mod r for a, b < r
KZG_HD constexpr void fr_add(fr& out, const fr& a, const fr& b) {
  uint32_t t[9] = {};
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
KZG_HD constexpr void fr_sub(fr& out, const fr& a, const fr& b) {
  uint32_t d[8] = {};
  uint32_t br = 0;
  for (int i = 0; i < 8; i++) {
    const uint64_t s = (uint64_t)a.v[i] - b.v[i] - br;  // wraps mod 2^64 on a borrow: bit 32 is then set
    d[i] = (uint32_t)s;
    br = (uint32_t)(s >> 32) & 1u;
  }
  uint32_t c = 0;  // a < b: the difference wrapped mod 2^256, and adding r wraps it back
  for (int i = 0; i < 8; i++) {
    const uint64_t s = (uint64_t)d[i] + (br ? FR_R[i] : 0u) + c;
    out.v[i] = (uint32_t)s;
    c = (uint32_t)(s >> 32);
  }
}

// R = 2^256 mod r (the Montgomery one) and R^2 mod r, by 256 and 512 doublings at compile time
struct fr_radix {
  uint32_t one[8], r2[8];
};
constexpr fr_radix fr_make_radix() {
  fr_radix k = {};
  fr x = {{1, 0, 0, 0, 0, 0, 0, 0}};
  for (int i = 0; i < 512; i++) {  // x = 2^(i + 1) mod r
    fr_add(x, x, x);
    if (i == 255)
      for (int j = 0; j < 8; j++) k.one[j] = x.v[j];
  }
  for (int j = 0; j < 8; j++) k.r2[j] = x.v[j];
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
KZG_HD void fr_load(fr& out, const fr& a) {
  fr r2;
  for (int i = 0; i < 8; i++) r2.v[i] = FR_RADIX.r2[i];
  fr_mul(out, a, r2);
}
// Store: Montgomery form -> the canonical value below r (8 LE words: 32 little-endian bytes), a * 1
KZG_HD void fr_store(fr& out, const fr& a) {
  fr one = {{1, 0, 0, 0, 0, 0, 0, 0}};
  fr_mul(out, a, one);
}

// ---------------------------------------------------------------- where the ABI units start from
// Elements are in Montgomery form; exponents are plain 256-bit integers.
KZG_HD fr fr_one() {
  fr o;
  for (int i = 0; i < 8; i++) o.v[i] = FR_RADIX.one[i];
  return o;
}
KZG_HD fr fr_from_u64(uint64_t a) {
  fr x = {{(uint32_t)a, (uint32_t)(a >> 32), 0, 0, 0, 0, 0, 0}};
  fr_load(x, x);
  return x;
}

// the integers r - d (d = 2: the exponent of the inverse) and (r - 1) >> k, k <= 32
KZG_HD constexpr fr fr_r_minus(uint32_t d) {
  fr e = {};
  int64_t br = -(int64_t)d;
  for (int i = 0; i < 8; i++) {
    const int64_t s = (int64_t)FR_R[i] + br;
    e.v[i] = (uint32_t)s;
    br = s >> 32;
  }
  return e;
}
KZG_HD constexpr fr fr_rm1_shr(uint32_t k) {
  const fr a = fr_r_minus(1);
  fr e = {};
  for (int i = 0; i < 8; i++) e.v[i] = (uint32_t)((((uint64_t)(i < 7 ? a.v[i + 1] : 0) << 32) | a.v[i]) >> k);
  return e;
}

KZG_HD fr fr_pow(const fr& base, const fr& e) {
  fr acc = fr_one();
  for (int b = 255; b >= 0; b--) {
    fr_mul(acc, acc, acc);
    if ((e.v[b >> 5] >> (b & 31)) & 1) fr_mul(acc, acc, base);
  }
  return acc;
}
KZG_HD fr fr_inv(const fr& a) { return fr_pow(a, fr_r_minus(2)); }  // 0 for a = 0

// w_m = 7^((r - 1) / 2^exp), exp <= 32: bellman's omega for the domain of size 2^exp (its
// root_of_unity = 7^((r-1)/2^32) squared 32 - exp times), and ark-poly's Radix2EvaluationDomain's
KZG_HD fr fr_domain_root(uint32_t exp) { return fr_pow(fr_from_u64(7), fr_rm1_shr(exp)); }

// 32 little-endian bytes, any 256-bit integer -> its residue; an element -> its canonical value as
// 32 little-endian or big-endian bytes
KZG_HD fr fr_from_le32(const uint8_t b[32]) {
  fr a;
  for (int k = 0; k < 8; k++)
    a.v[k] = (uint32_t)b[4 * k] | (uint32_t)b[4 * k + 1] << 8 | (uint32_t)b[4 * k + 2] << 16 |
             (uint32_t)b[4 * k + 3] << 24;
  fr_load(a, a);
  return a;
}
KZG_HD void fr_to_le32(uint8_t out[32], const fr& a) {
  fr c;
  fr_store(c, a);
  for (int i = 0; i < 32; i++) out[i] = (uint8_t)(c.v[i >> 2] >> (8 * (i & 3)));
}
KZG_HD void fr_to_be32(uint8_t out[32], const fr& a) {
  fr c;
  fr_store(c, a);
  for (int i = 0; i < 32; i++) out[31 - i] = (uint8_t)(c.v[i >> 2] >> (8 * (i & 3)));
}

// p[k] = x^(2^k), the table a kernel builds x^j from over j's bits
template <int N>
struct fr_powers {
  fr p[N];
};
template <int N>
KZG_HD void fr_fill_powers(fr (&p)[N], fr x) {
  for (int k = 0; k < N; k++) {
    p[k] = x;
    fr_mul(x, x, x);
  }
}

}  // namespace kzgpot
