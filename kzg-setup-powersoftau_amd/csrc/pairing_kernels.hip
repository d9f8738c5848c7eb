// Product of BLS12-381 pairings: prod_i e(P_i, Q_i)^d for ark-uncompressed G1 / G2
// records, d = KZGPOT_PAIRING_GT_POWER, and whether that product is one.
//
// Tower (ark-bls12-381's): Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v),
// xi = u + 1. An Fq12 element is six Fq2 coefficients b_e of w^e (w^6 = xi); it is stored in ark's
// order c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, which are the powers w^0, w^2, w^4, w^1, w^3, w^5.
//
// An Fq12 element is 168 words: a lane cannot hold several in registers. Every value of the
// computation therefore lives in a lane's CELLS in the workspace (one Fq2 of 28 words per cell, word-
// major across lanes so a wave's access to one word is contiguous), and the arithmetic is a sequence
// of calls that read one or two cells into registers and write one back (c_mul, c_sqr, c_add ...), or
// loop over the cells of two elements with two Fq2 accumulators in registers (x_mul, x_mul_line). Every
// such function is compiled once, not inlined: the Fq2 multiply is about 1,200 mads, and the Miller
// loop and the exponentiation call it from a hundred places. LDS cannot take the state instead: the
// Miller loop's 29 cells are 3.2 KB per lane, 208 KB for one wave.
//
// All values between calls are "reduced" (fp381.hpp: normalized limbs, value < 2 p): products leave
// f_mul / f_sqr below 1.01 p, sums and differences go through fp_add_red / fp_sub_red. No lazily
// bounded intermediate exists outside f_mul and f_sqr themselves.
//
//   k_pair_miller  one lane per pair: the records' checks (as the MSM's load: 3 / 6, smallest index
//                  along g1 then g2), then the Miller loop over |x| on the M-type twist in homogeneous
//                  projective coordinates, the line's three coefficients computed on the fly
//                  (Costello, Lange, Naehrig: "Faster pairing computations on curves with high-degree
//                  twists", as ark-ec's bls12 doubling_step / addition_step) and multiplied into the
//                  accumulator as the sparse element l0 + l1 w^2 + l2 w^3. A pair with a point at
//                  infinity contributes 1.
//   k_pair_tree    the product of the lanes' Miller values: a block multiplies 256 of them in eight
//                  levels, one launch per factor of 256 in the pair count.
//   k_pair_final   one lane: conjugation (x < 0), the easy part f^((p^6 - 1)(p^2 + 1)) by one Fq12
//                  inversion and Frobenius maps, the hard part m^((x - 1)^2 (x + p)(x^2 + p^2 - 1)) m^3
//                  = m^(3 (p^4 - p^2 + 1) / r) (Hayashida, Hayasaka, Teruya: "Efficient final
//                  exponentiation via cyclotomic structure for pairings over families of elliptic
//                  curves") by five exponentiations by |x|, the canonical bytes and the comparison
//                  with one. Nothing is written once the key reports a rejected record.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec.hpp"
#include "group_parts.hpp"

namespace kzgpot {
namespace {

static_assert(KZGPOT_PAIRING_GT_POWER == 3, "the hard part below computes the cube");

constexpr int kCellWords = 2 * NL;
static_assert(kCellWords * 4 == kPairCellBytes, "a cell is one Fq2 (plans.hpp)");

// A lane's cells: word w of cell c at p[(c * kCellWords + w) * stride]
struct Cells {
  uint32_t* p;
  uint64_t stride;
};

KZG_DEV void ld(fp2& a, Cells m, int c) {
  const uint32_t* s = m.p + (uint64_t)c * kCellWords * m.stride;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    a.c0.v[k] = s[(uint64_t)k * m.stride];
    a.c1.v[k] = s[(uint64_t)(NL + k) * m.stride];
  }
}
KZG_DEV void st(Cells m, int c, const fp2& a) {
  uint32_t* d = m.p + (uint64_t)c * kCellWords * m.stride;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    d[(uint64_t)k * m.stride] = a.c0.v[k];
    d[(uint64_t)(NL + k) * m.stride] = a.c1.v[k];
  }
}

// ---------------------------------------------------------------- Fq2 on registers, reduced in and out
KZG_DEV void f2_add(fp2& r, const fp2& a, const fp2& b) {
  fp_add_red(r.c0, a.c0, b.c0);
  fp_add_red(r.c1, a.c1, b.c1);
}
KZG_DEV void f2_sub(fp2& r, const fp2& a, const fp2& b) {
  fp_sub_red(r.c0, a.c0, b.c0);
  fp_sub_red(r.c1, a.c1, b.c1);
}
KZG_DEV void f2_mul_xi(fp2& r, const fp2& a) {  // (a0 + a1 u)(1 + u) = (a0 - a1) + (a0 + a1) u
  fp t;
  fp_sub_red(t, a.c0, a.c1);
  fp_add_red(r.c1, a.c0, a.c1);
  r.c0 = t;
}
KZG_DEV void f2_zero(fp2& r) {
  fp_zero(r.c0);
  fp_zero(r.c1);
}

// ---------------------------------------------------------------- Fq2 on cells
#define KZG_CELL_FN __device__ __noinline__

KZG_CELL_FN void c_mul(Cells m, int d, int a, int b) {
  fp2 x, y;
  ld(x, m, a);
  ld(y, m, b);
  f_mul(x, x, y);
  st(m, d, x);
}
KZG_CELL_FN void c_sqr(Cells m, int d, int a) {
  fp2 x;
  ld(x, m, a);
  f_sqr(x, x);
  st(m, d, x);
}
KZG_CELL_FN void c_add(Cells m, int d, int a, int b) {
  fp2 x, y;
  ld(x, m, a);
  ld(y, m, b);
  f2_add(x, x, y);
  st(m, d, x);
}
KZG_CELL_FN void c_sub(Cells m, int d, int a, int b) {
  fp2 x, y;
  ld(x, m, a);
  ld(y, m, b);
  f2_sub(x, x, y);
  st(m, d, x);
}
KZG_CELL_FN void c_neg(Cells m, int d, int a) {
  fp2 x;
  ld(x, m, a);
  fp2_neg_red(x, x);
  st(m, d, x);
}
KZG_CELL_FN void c_mul_xi(Cells m, int d, int a) {
  fp2 x;
  ld(x, m, a);
  f2_mul_xi(x, x);
  st(m, d, x);
}
KZG_CELL_FN void c_half(Cells m, int d, int a) {  // a / 2, as a multiplication by Montgomery 1/2
  fp2 x;
  fp h;
  ld(x, m, a);
  fp_set(h, FP_INV2);
  fp_mul(x.c0, x.c0, h);
  fp_mul(x.c1, x.c1, h);
  st(m, d, x);
}
// a times component `which` (an Fq element) of cell s
KZG_CELL_FN void c_mul_fq(Cells m, int d, int a, int s, int which) {
  fp2 x, y;
  ld(x, m, a);
  ld(y, m, s);
  const fp& f = which ? y.c1 : y.c0;
  fp_mul(x.c0, x.c0, f);
  fp_mul(x.c1, x.c1, f);
  st(m, d, x);
}
KZG_CELL_FN void c_inv(Cells m, int d, int a) {
  fp2 x;
  ld(x, m, a);
  f_inv(x, x);
  st(m, d, x);
}
// n cells, possibly from another lane's
KZG_CELL_FN void c_copy(Cells md, int d, Cells ma, int a, int n) {
#pragma unroll 1
  for (int k = 0; k < n; k++) {
    fp2 x;
    ld(x, ma, a + k);
    st(md, d + k, x);
  }
}
KZG_CELL_FN void c_set_one(Cells m, int d, int n) {  // the element 1 of n cells
  fp2 x;
  f_one(x);
#pragma unroll 1
  for (int k = 0; k < n; k++) {
    st(m, d + k, x);
    fp_zero(x.c0);
  }
}

// ---------------------------------------------------------------- Fq6 and Fq12 on cells
// the cell of the coefficient of X^e: Fq12 (n = 6, X = w) in ark's order, Fq6 (n = 3, X = v) in sequence
KZG_DEV int xcell(int n, int base, int e) { return n == 6 ? base + (e & 1) * 3 + (e >> 1) : base + e; }

// d = a b in Fq2[X] / (X^n - xi): coefficient k is sum_{i + j = k} a_i b_j + xi sum_{i + j = k + n} a_i b_j.
// square: b is a, and each cross product is taken once and doubled. d's cells overlap neither a's nor b's.
KZG_CELL_FN void x_mul(Cells md, int d, Cells ma, int a, Cells mb, int b, int n, bool square) {
#pragma unroll 1
  for (int k = 0; k < n; k++) {
    fp2 lo, hi;
    f2_zero(lo);
    f2_zero(hi);
#pragma unroll 1
    for (int i = 0; i < n; i++) {
      const bool wrap = i > k;
      const int j = wrap ? k - i + n : k - i;
      if (square && i > j) continue;
      fp2 x, t;
      ld(x, ma, xcell(n, a, i));
      if (square && i == j) {
        f_sqr(t, x);
      } else {
        fp2 y;
        ld(y, mb, xcell(n, b, j));
        f_mul(t, x, y);
        if (square) f2_add(t, t, t);
      }
      if (wrap) f2_add(hi, hi, t);
      else f2_add(lo, lo, t);
    }
    f2_mul_xi(hi, hi);
    f2_add(lo, lo, hi);
    st(md, xcell(n, d, k), lo);
  }
}
// d = a (l0 + l1 w^2 + l2 w^3) in Fq12, the line's coefficients in cells l, l + 1, l + 2 (ark's mul_by_014)
KZG_CELL_FN void x_mul_line(Cells m, int d, int a, int l) {
#pragma unroll 1
  for (int k = 0; k < 6; k++) {
    fp2 lo, hi;
    f2_zero(lo);
    f2_zero(hi);
#pragma unroll 1
    for (int t = 0; t < 3; t++) {
      const int e = t ? t + 1 : 0;
      const bool wrap = e > k;
      const int i = wrap ? k - e + 6 : k - e;
      fp2 x, y;
      ld(x, m, xcell(6, a, i));
      ld(y, m, l + t);
      f_mul(x, x, y);
      if (wrap) f2_add(hi, hi, x);
      else f2_add(lo, lo, x);
    }
    f2_mul_xi(hi, hi);
    f2_add(lo, lo, hi);
    st(m, xcell(6, d, k), lo);
  }
}

struct FrobTable {
  uint32_t v[2][6][2][NL];
  constexpr FrobTable() : v{} {
    for (int k = 0; k < 2; k++)
      for (int e = 0; e < 6; e++)
        for (int c = 0; c < 2; c++)
          for (int i = 0; i < NL; i++) v[k][e][c][i] = FP12_FROB[k][e][c][i];
  }
};
__constant__ constexpr FrobTable kFrob{};

// d = a^(p^k), k = 1 or 2: conj^k of each coefficient times xi^(e (p^k - 1) / 6); d may be a
KZG_CELL_FN void x_frob(Cells m, int d, int a, int k) {
#pragma unroll 1
  for (int e = 0; e < 6; e++) {
    fp2 x, g;
    ld(x, m, xcell(6, a, e));
    if (k & 1) {
      fp z;
      fp_zero(z);
      fp_sub_red(x.c1, z, x.c1);
    }
#pragma unroll
    for (int i = 0; i < NL; i++) {
      g.c0.v[i] = kFrob.v[k - 1][e][0][i];
      g.c1.v[i] = kFrob.v[k - 1][e][1][i];
    }
    f_mul(x, x, g);
    st(m, xcell(6, d, e), x);
  }
}
// d = conj(a) = a^(p^6): the coefficients of the odd powers of w negated; d may be a
__device__ void x_conj(Cells m, int d, int a) {
  if (d != a) c_copy(m, d, m, a, 3);
  for (int k = 3; k < 6; k++) c_neg(m, d + k, a + k);
}

// d = 1 / a in Fq6 (three cells each); s: five free cells. d may not be a.
__device__ void x6_inv(Cells m, int d, int a, int s) {
  // c0 = a0^2 - xi a1 a2, c1 = xi a2^2 - a0 a1, c2 = a1^2 - a0 a2
  c_sqr(m, s + 0, a + 0);
  c_mul(m, s + 3, a + 1, a + 2);
  c_mul_xi(m, s + 3, s + 3);
  c_sub(m, s + 0, s + 0, s + 3);
  c_sqr(m, s + 1, a + 2);
  c_mul_xi(m, s + 1, s + 1);
  c_mul(m, s + 3, a + 0, a + 1);
  c_sub(m, s + 1, s + 1, s + 3);
  c_sqr(m, s + 2, a + 1);
  c_mul(m, s + 3, a + 0, a + 2);
  c_sub(m, s + 2, s + 2, s + 3);
  // t = a0 c0 + xi (a2 c1 + a1 c2)
  c_mul(m, s + 3, a + 2, s + 1);
  c_mul(m, s + 4, a + 1, s + 2);
  c_add(m, s + 3, s + 3, s + 4);
  c_mul_xi(m, s + 3, s + 3);
  c_mul(m, s + 4, a + 0, s + 0);
  c_add(m, s + 3, s + 3, s + 4);
  c_inv(m, s + 3, s + 3);
  for (int k = 0; k < 3; k++) c_mul(m, d + k, s + k, s + 3);
}
// d = 1 / a in Fq12: (a0 - a1 w) / (a0^2 - v a1^2); s: 17 free cells. d may not be a.
__device__ void x12_inv(Cells m, int d, int a, int s) {
  x_mul(m, s + 0, m, a, m, a, 3, true);          // a0^2
  x_mul(m, s + 3, m, a + 3, m, a + 3, 3, true);  // a1^2 = (t0, t1, t2); v a1^2 = (xi t2, t0, t1)
  c_mul_xi(m, s + 6, s + 5);
  c_sub(m, s + 0, s + 0, s + 6);
  c_sub(m, s + 1, s + 1, s + 3);
  c_sub(m, s + 2, s + 2, s + 4);
  x6_inv(m, s + 9, s + 0, s + 12);
  x_mul(m, d, m, a, m, s + 9, 3, false);
  x_mul(m, d + 3, m, a + 3, m, s + 9, 3, false);
  for (int k = 3; k < 6; k++) c_neg(m, d + k, d + k);
}

// ---------------------------------------------------------------- Miller loop
// a lane's cells (kPairLaneCells of them, plans.hpp)
enum : int {
  F = 0,      // the accumulator, 6 cells
  G = 6,      // its square / the other side of a product, 6 cells
  LINE = 12,  // the line's coefficients of w^0, w^2, w^3
  TX = 15, TY = 16, TZ = 17,  // the running point [m] Q on the twist, homogeneous projective
  QX = 18, QY = 19,           // Q
  PXY = 20,                   // P: x in component 0, y in component 1
  S0 = 21, S1, S2, S3, S4, S5, S6, S7,
  kMillerCells
};
static_assert(kMillerCells == kPairLaneCells, "the plan's cells per lane (plans.hpp)");

// T <- 2 T; the line: tangent at T, evaluated at P
__device__ void miller_double(Cells m) {
  c_mul(m, S0, TX, TY);
  c_half(m, S0, S0);    // a = X Y / 2
  c_sqr(m, S1, TY);     // b = Y^2
  c_sqr(m, S2, TZ);     // c = Z^2
  c_add(m, S3, S2, S2);
  c_add(m, S3, S3, S2);
  c_add(m, S3, S3, S3);
  c_add(m, S3, S3, S3);
  c_mul_xi(m, S3, S3);  // e = 3 b' c, b' = 4 xi
  c_add(m, S4, S3, S3);
  c_add(m, S4, S4, S3);  // f = 3 e
  c_add(m, S5, S1, S4);
  c_half(m, S5, S5);     // g = (b + f) / 2
  c_add(m, S6, TY, TZ);
  c_sqr(m, S6, S6);
  c_sub(m, S6, S6, S1);
  c_sub(m, S6, S6, S2);  // h = (Y + Z)^2 - b - c = 2 Y Z
  c_sub(m, LINE, S3, S1);  // l0 = e - b
  c_sqr(m, S7, TX);      // j = X^2
  c_sqr(m, S3, S3);      // e^2
  c_sub(m, S4, S1, S4);
  c_mul(m, TX, S0, S4);  // X3 = a (b - f)
  c_sqr(m, S5, S5);
  c_add(m, S4, S3, S3);
  c_add(m, S4, S4, S3);
  c_sub(m, TY, S5, S4);  // Y3 = g^2 - 3 e^2
  c_mul(m, TZ, S1, S6);  // Z3 = b h
  c_add(m, S4, S7, S7);
  c_add(m, S4, S4, S7);
  c_mul_fq(m, LINE + 1, S4, PXY, 0);  // l1 = 3 j xP
  c_neg(m, S6, S6);
  c_mul_fq(m, LINE + 2, S6, PXY, 1);  // l2 = -h yP
}
// T <- T + Q; the line through T and Q, evaluated at P
__device__ void miller_add(Cells m) {
  c_mul(m, S0, QY, TZ);
  c_sub(m, S0, TY, S0);  // theta = Y - qy Z
  c_mul(m, S1, QX, TZ);
  c_sub(m, S1, TX, S1);  // lambda = X - qx Z
  c_sqr(m, S2, S0);      // c = theta^2
  c_sqr(m, S3, S1);      // d = lambda^2
  c_mul(m, S4, S1, S3);  // e = lambda d
  c_mul(m, S2, TZ, S2);  // f = Z c
  c_mul(m, S3, TX, S3);  // g = X d
  c_add(m, S5, S4, S2);
  c_sub(m, S5, S5, S3);
  c_sub(m, S5, S5, S3);  // h = e + f - 2 g
  c_mul(m, TX, S1, S5);  // X3 = lambda h
  c_sub(m, S3, S3, S5);
  c_mul(m, S3, S0, S3);
  c_mul(m, S6, S4, TY);
  c_sub(m, TY, S3, S6);  // Y3 = theta (g - h) - e Y
  c_mul(m, TZ, TZ, S4);  // Z3 = Z e
  c_mul(m, S2, S0, QX);
  c_mul(m, S3, S1, QY);
  c_sub(m, LINE, S2, S3);  // l0 = theta qx - lambda qy
  c_neg(m, S0, S0);
  c_mul_fq(m, LINE + 1, S0, PXY, 0);  // l1 = -theta xP
  c_mul_fq(m, LINE + 2, S1, PXY, 1);  // l2 = lambda yP
}

// indices reported: key_bias + i for g1[i], key_bias + k + i for g2[i]
__global__ void __launch_bounds__(kPairMillerBlock) k_pair_miller(const uint4* __restrict__ g1, const uint4* __restrict__ g2,
                                                                   uint64_t k, uint32_t* cells, uint64_t stride,
                                                                   unsigned long long* key, uint64_t key_bias) {
  const uint64_t i = (uint64_t)blockIdx.x * kPairMillerBlock + threadIdx.x;
  if (i >= k) return;
  const Cells m{cells + i, stride};
  bool skip;
  {
    fp px, py;
    bool inf1;
    const int st1 = ark_record_decode(px, py, inf1, g1 + 6 * i);
    report(key_bias + i, st1, key, nullptr);
    fp2 q;
    q.c0 = px, q.c1 = py;
    st(m, PXY, q);
    skip = st1 != 0 || inf1;
  }
  {
    fp2 qx, qy;
    bool inf2;
    const int st2 = ark_record_decode(qx, qy, inf2, g2 + 12 * i);
    report(key_bias + k + i, st2, key, nullptr);
    st(m, QX, qx);
    st(m, QY, qy);
    st(m, TX, qx);
    st(m, TY, qy);
    skip = skip || st2 != 0 || inf2;
  }
  c_set_one(m, F, 6);
  if (skip) return;
  c_set_one(m, TZ, 1);
#pragma unroll 1
  for (int b = BLS_ABS_U_BITS - 2; b >= 0; b--) {
    x_mul(m, G, m, F, m, F, 6, true);
    miller_double(m);
    x_mul_line(m, F, G, LINE);
    if ((BLS_ABS_U >> b) & 1) {
      miller_add(m);
      x_mul_line(m, G, F, LINE);
      c_copy(m, F, m, G, 6);
    }
  }
}

// `count` live values, the g-th in the F cells of lane g step; block b leaves the product of its 256
// in lane 256 b step
__global__ void __launch_bounds__(256) k_pair_tree(uint32_t* cells, uint64_t stride, uint64_t count, uint64_t step) {
  const uint32_t tid = threadIdx.x;
  const uint64_t g = (uint64_t)blockIdx.x * 256 + tid;
  const Cells mine{cells + g * step, stride};
#pragma unroll 1
  for (uint32_t s = 1; s < 256; s <<= 1) {
    if ((tid & (2 * s - 1)) == 0 && tid + s < 256 && g + s < count) {
      const Cells other{cells + (g + s) * step, stride};
      x_mul(mine, G, mine, F, other, F, 6, false);
      c_copy(mine, F, mine, G, 6);
    }
    __threadfence_block();
    __syncthreads();
  }
}

// ---------------------------------------------------------------- final exponentiation
// the one lane's cells: six Fq12 values and the inversion's scratch
enum : int { A = 0, B = 6, C = 12, D = 18, E = 24, T = 30, SCR = 36, kFinalCells = SCR + 17 };
static_assert(kFinalCells <= kPairFinalCells, "the plan's cells of the final exponentiation (plans.hpp)");

__device__ void x12_mul(Cells m, int d, int a, int b) { x_mul(m, d, m, a, m, b, 6, false); }
__device__ void x12_sqr(Cells m, int d, int a) { x_mul(m, d, m, a, m, a, 6, true); }
// d = a^|x| by square and multiply from the top bit; d is neither a nor T
__device__ void x12_pow_x(Cells m, int d, int a) {
  int cur = d, oth = T;
  c_copy(m, cur, m, a, 6);
#pragma unroll 1
  for (int b = BLS_ABS_U_BITS - 2; b >= 0; b--) {
    x12_sqr(m, oth, cur);
    int t = cur;
    cur = oth, oth = t;
    if ((BLS_ABS_U >> b) & 1) {
      x12_mul(m, oth, cur, a);
      t = cur;
      cur = oth, oth = t;
    }
  }
  if (cur != d) c_copy(m, d, m, cur, 6);
}

__global__ void __launch_bounds__(64) k_pair_final(const uint32_t* lane0, uint64_t stride, uint64_t k, uint32_t* fcells,
                                                   uint4* out, const unsigned long long* key) {
  if (threadIdx.x != 0 || rejected(key)) return;
  const Cells m{fcells, 1};
  if (k) c_copy(m, A, Cells{const_cast<uint32_t*>(lane0), stride}, F, 6);
  else c_set_one(m, A, 6);
  x_conj(m, A, A);  // x < 0: the Miller value of the loop over |x|, inverted up to what the easy part removes
  // easy part: m = f^((p^6 - 1)(p^2 + 1))
  x_conj(m, B, A);
  x12_inv(m, C, A, SCR);
  x12_mul(m, D, B, C);
  x_frob(m, B, D, 2);
  x12_mul(m, A, B, D);
  // hard part, m in the cyclotomic subgroup (its inverse is its conjugate), x = -|x|:
  // t0 = m^(x - 1)
  x12_pow_x(m, B, A);
  x_conj(m, B, B);
  x_conj(m, C, A);
  x12_mul(m, D, B, C);
  // t1 = t0^(x - 1)
  x12_pow_x(m, B, D);
  x_conj(m, B, B);
  x_conj(m, C, D);
  x12_mul(m, E, B, C);
  // t2 = t1^(x + p)
  x12_pow_x(m, B, E);
  x_conj(m, B, B);
  x_frob(m, C, E, 1);
  x12_mul(m, D, B, C);
  // t3 = t2^(x^2 + p^2 - 1)
  x12_pow_x(m, B, D);
  x12_pow_x(m, C, B);
  x_frob(m, B, D, 2);
  x12_mul(m, E, C, B);
  x_conj(m, B, D);
  x12_mul(m, C, E, B);
  // t3 m^3
  x12_sqr(m, B, A);
  x12_mul(m, D, B, A);
  x12_mul(m, E, C, D);
  // canonical bytes in ark's order, and the comparison with one
  uint32_t diff = 0;
#pragma unroll 1
  for (int c = 0; c < 6; c++) {
    fp2 x;
    ld(x, m, E + c);
    fp_from_mont(x.c0, x.c0);
    fp_from_mont(x.c1, x.c1);
    store_canon(out + 6 * c, x.c0);
    store_canon(out + 6 * c + 3, x.c1);
#pragma unroll
    for (int i = 0; i < NL; i++) diff |= (x.c0.v[i] ^ (c == 0 && i == 0 ? 1u : 0u)) | x.c1.v[i];
  }
  *(uint32_t*)(out + 36) = diff == 0 ? 1u : 0u;
}

}  // namespace

hipError_t launch_pairing_product(const void* d_g1, const void* d_g2, uint64_t k, void* d_out, void* d_work,
                                  unsigned long long* d_key, uint64_t key_bias, hipStream_t stream) {
  const PairingPlan p = pairing_plan(k);
  if (!p.ok) return hipErrorInvalidValue;
  uint32_t* cells = (uint32_t*)((uint8_t*)d_work + p.lanes);
  uint32_t* fcells = (uint32_t*)((uint8_t*)d_work + p.final_cells);
  if (k)
    hipLaunchKernelGGL(k_pair_miller, dim3(grid_for(k, kPairMillerBlock)), dim3(kPairMillerBlock), 0, stream,
                       (const uint4*)d_g1, (const uint4*)d_g2, k, cells, p.stride, d_key, key_bias);
  for (uint32_t l = 0; l < p.nlevels; l++)
    hipLaunchKernelGGL(k_pair_tree, dim3(p.level[l].blocks), dim3(256), 0, stream, cells, p.stride, p.level[l].count,
                       p.level[l].step);
  hipLaunchKernelGGL(k_pair_final, dim3(1), dim3(64), 0, stream, (const uint32_t*)cells, p.stride, k, fcells,
                     (uint4*)d_out, (const unsigned long long*)d_key);
  return hipGetLastError();
}

}  // namespace kzgpot
