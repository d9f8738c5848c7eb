// The pairing product's device functions on cells, included by pairing_kernels.hip
// (k_pair_miller, k_pair_final and the launch) and, in the test build, by pairing_hooks.hip, which
// runs one of them per lane on caller-supplied cells: both compile this text.
//   cells     a lane's Fq2 values in the workspace, ld / st, the c_* operations on them
//   elements  Fq6 / Fq12 over cells: x_mul, x_mul_line, x_frob, x_conj, x6_inv, x12_inv, x12_pow_x
//   Miller    the lane's cell layout, the doubling and the addition step
//   tree      k_pair_tree and launch_pair_tree, the one loop over its levels
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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "codec.hpp"
#include "group_parts.hpp"

namespace kzgpot {
namespace {

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

// ---------------------------------------------------------------- product tree
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
// the plan's levels, one launch each: lane 0's F cells then hold the product of the p.k lanes' F
// values (nothing is launched for p.k <= 1); `stride` lanes per word, p.k of them live
inline void launch_pair_tree(const PairingPlan& p, uint32_t* cells, uint64_t stride, hipStream_t stream) {
  for (uint32_t l = 0; l < p.nlevels; l++)
    hipLaunchKernelGGL(k_pair_tree, dim3(p.level[l].blocks), dim3(256), 0, stream, cells, stride, p.level[l].count,
                       p.level[l].step);
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

}  // namespace
}  // namespace kzgpot
