// BLS12-381 scalar field Fr (the group order r), stated once for the host and the device: 8 x 32-bit
// little-endian words, Montgomery form with R = 2^256, one CIOS multiply. The ABI units start from
// the host helpers at the end (phase2.hip: the domain root, the powers w^(+-2^k), 1/m; open.hip: the
// powers z^(2^k)); the kernels use the arithmetic (fft_kernels.hip: k_fft_twiddles builds w^j from
// those powers with poly_parts.hpp's ladder; poly_kernels.hip: the polynomial division of KZG10
// open; ntt_kernels.hip: the NTT's butterflies, and eval_kernels.hip: the batch inversion and the
// division in evaluation form, the places where these multiplies are the hot path; evals.hip starts
// that division from fr_eval_setup). Elsewhere nothing here is hot: ~31 multiplies per twiddle
// against the 254 point doublings the twiddle then drives.
//
// Plain C++17 unless the compiler is hipcc, so a host program can include this file alone
// (tests/host_units/fr_units.cpp and eval_units.cpp, built by g++ with and without sanitizers).
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
KZG_HD fr fr_zero() { return fr{{0, 0, 0, 0, 0, 0, 0, 0}}; }
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

// ---------------------------------------------------------------- evaluation form (evals.hip)
KZG_HD bool fr_is_zero(const fr& a) {
  uint32_t any = 0;
  for (int i = 0; i < 8; i++) any |= a.v[i];
  return any == 0;
}
// The inverse of a (Montgomery form in and out; 0 for 0) without a multiplication: Kaliski's almost
// inverse ("The Montgomery inverse and its applications", 1995), then doublings; 512 steps in all
// whatever a is. The binary steps work on u, v, r, s from (the modulus, a, 0, 1) and keep
// u s + v r = the modulus, so s <= the modulus while u >= 1 and r <= the modulus while v >= 1, and
// the step that leaves v = 0 doubles r once more: every value stays below 2^256 (the modulus has 255
// bits). After those k steps (255 <= k <= 510) the modulus minus r is a^-1 2^k, and the remaining
// 512 - k steps double it: a^-1 2^512 = a^-1 R^2 is the Montgomery form of the inverse of the value
// that a stands for. A step is a few word-wide shifts, one comparison and one addition or
// subtraction; fr_inv's ladder is 383 multiplications.
KZG_HD fr fr_inv_binary(const fr& a) {
  uint32_t u[8], v[8], r[8], s[8];
  for (int i = 0; i < 8; i++) u[i] = FR_R[i], v[i] = a.v[i], r[i] = 0, s[i] = i == 0;
  fr x = fr_zero();
  bool reduced = fr_is_zero(a);  // x holds a^-1 2^(steps so far)
  auto halve = [](uint32_t (&w)[8]) {
    for (int i = 0; i < 8; i++) w[i] = (w[i] >> 1) | (i < 7 ? w[i + 1] << 31 : 0u);
  };
  auto twice = [](uint32_t (&w)[8]) {
    for (int i = 7; i >= 0; i--) w[i] = (w[i] << 1) | (i > 0 ? w[i - 1] >> 31 : 0u);
  };
  auto add = [](uint32_t (&w)[8], const uint32_t (&y)[8]) {  // below 2^256: no carry out
    uint64_t c = 0;
    for (int i = 0; i < 8; i++) {
      c += (uint64_t)w[i] + y[i];
      w[i] = (uint32_t)c;
      c >>= 32;
    }
  };
  auto sub = [](uint32_t (&w)[8], const uint32_t (&y)[8]) -> bool {  // w -= y; true: it wrapped (w < y)
    uint32_t br = 0;
    for (int i = 0; i < 8; i++) {
      const uint64_t d = (uint64_t)w[i] - y[i] - br;
      w[i] = (uint32_t)d;
      br = (uint32_t)(d >> 32) & 1u;
    }
    return br != 0;
  };
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll 1
#endif
  for (int step = 0; step < 512; step++) {
    if (reduced) {
      fr_add(x, x, x);
      continue;
    }
    if (!(u[0] & 1)) {
      halve(u), twice(s);
    } else if (!(v[0] & 1)) {
      halve(v), twice(r);
    } else {
      uint32_t d[8];
      for (int i = 0; i < 8; i++) d[i] = u[i];
      if (!sub(d, v)) {  // u >= v; equal only when both are 1, the last step
        bool zero = true;
        for (int i = 0; i < 8; i++) zero = zero && d[i] == 0;
        if (zero) {  // v - u = 0
          for (int i = 0; i < 8; i++) v[i] = 0;
          add(s, r), twice(r);
        } else {
          for (int i = 0; i < 8; i++) u[i] = d[i];
          halve(u), add(r, s), twice(s);
        }
      } else {
        sub(v, u);
        halve(v), add(s, r), twice(r);
      }
    }
    bool done = true;
    for (int i = 0; i < 8; i++) done = done && v[i] == 0;
    if (done) {  // r < 2 modulus -> the modulus - (r mod modulus)
      uint32_t t[9];
      for (int i = 0; i < 8; i++) t[i] = r[i];
      t[8] = 0;
      fr rr;
      fr_cond_sub(rr, t);
      fr_sub(x, fr_zero(), rr);
      reduced = true;
    }
  }
  return x;
}

// x^(2^k) by k squarings: z^n for the domain of size n = 2^k
KZG_HD fr fr_pow_2k(fr x, uint32_t k) {
  for (uint32_t i = 0; i < k; i++) fr_mul(x, x, x);
  return x;
}
// 1 / 2^exp, exp < 64
KZG_HD fr fr_inv_2k(uint32_t exp) { return fr_inv(fr_from_u64((uint64_t)1 << exp)); }
// What the division in evaluation form reads for the domain of size n = 2^exp <= 2^26 and a point z
// (any 256-bit integer): pw[k] = w^(2^k) for w = fr_domain_root(exp) (1 from k = exp on), z, and the
// barycentric factor (z^n - 1) / n, which is zero exactly where z lies on the domain. Montgomery form.
constexpr int kEvalPowers = 26;
struct fr_eval_scalars {
  fr pw[kEvalPowers];
  fr z, scale;
};
KZG_HD void fr_eval_setup(fr_eval_scalars& sc, uint32_t exp, const uint8_t z_le32[32]) {
  fr_fill_powers(sc.pw, fr_domain_root(exp));
  sc.z = fr_from_le32(z_le32);
  fr zn1;
  fr_sub(zn1, fr_pow_2k(sc.z, exp), fr_one());
  fr_mul(sc.scale, zn1, fr_inv_2k(exp));
}

}  // namespace kzgpot
