// Product of BLS12-381 pairings: prod_i e(P_i, Q_i)^d for ark-uncompressed G1 / G2
// records, d = KZGPOT_PAIRING_GT_POWER, and whether that product is one.
//
// Tower (ark-bls12-381's): Fq2 = Fq[u]/(u^2 + 1), Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v),
// xi = u + 1. An Fq12 element is six Fq2 coefficients b_e of w^e (w^6 = xi); it is stored in ark's
// order c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, which are the powers w^0, w^2, w^4, w^1, w^3, w^5.
//
// The functions on cells (c_*, x_*, the two Miller steps, the product tree with its level loop) are
// pairing_parts.hpp, which says where the Fq12 state lives and what "reduced" means between calls; the
// test build's pairing_hooks.hip runs each of them per lane on supplied cells.
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
#include "pairing_parts.hpp"

namespace kzgpot {
namespace {

static_assert(KZGPOT_PAIRING_GT_POWER == 3, "the hard part below computes the cube");

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
  launch_pair_tree(p, cells, p.stride, stream);
  hipLaunchKernelGGL(k_pair_final, dim3(1), dim3(64), 0, stream, (const uint32_t*)cells, p.stride, k, fcells,
                     (uint4*)d_out, (const unsigned long long*)d_key);
  return hipGetLastError();
}

}  // namespace kzgpot
