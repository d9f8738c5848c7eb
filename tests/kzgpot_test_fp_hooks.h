/*
 * Test-only entry point of libkzgpot_test.so (kzg-setup-powersoftau_amd/Makefile, built with
 * -DKZGPOT_TEST_HOOKS) for the radix-2^28 / 2^29 field core, beside tests/kzgpot_test_f30_hooks.h.
 * The product library (libkzgpot.so) exports none of this.
 */
#ifndef KZGPOT_TEST_FP_HOOKS_H
#define KZGPOT_TEST_FP_HOOKS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* One function of the limb core (csrc/fp381.hpp fp_*, the Fp2 f_mul / f_sqr, and the 14 x 28 <-> 13 x 30
 * conversions) per GPU lane in blocks of 256 lanes (csrc/fp_hooks.hip): r = op(in[0], .., in[5]).
 * Operands and the result are lane-major uint32 arrays, lane i at [w i, w i + w) with the width w
 *   NL limbs (14 for BLS12-381, 9 for BN254) for a field element,
 *   NW words (12 / 8) for FROM_WORDS' operand and TO_WORDS' result,
 *   13 int32 digits, as their 32 bits, where an operand or the result is an f30,
 *   2 NL for the Fp2 results (c0, then c1), and 1 word, 0 or 1, for a predicate.
 * Operands an op does not take may be NULL. The limbs are whatever the caller supplies: keeping them
 * inside the functions' stated operand bounds is the caller's business.
 * field: KZGPOT_FP_BLS for every op; KZGPOT_FP_BN254 for MUL, SQR, ADD, EQ, IS_ZERO, FROM_WORDS,
 * TO_WORDS, TO_MONT, FROM_MONT, NEG_CANON, LT_CANON and SUBK / NEGK of KB_EQ (what bn254_kernels.hip
 * uses). Returns 0 or a negative KZGPOT_E_*. */
#define KZGPOT_FP_BLS 0
#define KZGPOT_FP_BN254 1

#define KZGPOT_FP_MUL 0          /* a b R^-1 */
#define KZGPOT_FP_SQR 1          /* a^2 R^-1 */
#define KZGPOT_FP_MUL_SUM2 2     /* (a b + c d) R^-1 */
#define KZGPOT_FP_MUL_SUM3 3     /* (a b + c d + e f) R^-1 */
#define KZGPOT_FP_MUL_ADDSQR8 5  /* fp_mul_add8sqr: (a b + 8 c^2) R^-1; 4 is not used */
#define KZGPOT_FP_NORM 6
#define KZGPOT_FP_HALF 7
#define KZGPOT_FP_REDUCE_ONCE 8
#define KZGPOT_FP_REDUCE_CANON 9
#define KZGPOT_FP_CANON 10
#define KZGPOT_FP_IS_ZERO 11   /* predicate */
#define KZGPOT_FP_EQ 12        /* predicate, a == b */
#define KZGPOT_FP_LT_CANON 13  /* predicate, a < b */
#define KZGPOT_FP_NEG_CANON 14
#define KZGPOT_FP_COND_SUB_2P 15
#define KZGPOT_FP_ADD_RED 16
#define KZGPOT_FP_SUB_RED 17
#define KZGPOT_FP_F2_MUL 18  /* f_mul(fp2): operands a.c0, a.c1, b.c0, b.c1 */
#define KZGPOT_FP_F2_SQR 19  /* f_sqr(fp2): operands a.c0, a.c1 */
#define KZGPOT_FP_FROM_WORDS 20
#define KZGPOT_FP_TO_WORDS 21
#define KZGPOT_FP_TO_MONT 22
#define KZGPOT_FP_FROM_MONT 23
#define KZGPOT_FP_ADD 24
#define KZGPOT_FP_F30_IS_ZERO 25  /* f30_is_zero<F30_ZK> (curve.hpp), predicate */
#define KZGPOT_FP_F30_FROM_FP 26
#define KZGPOT_FP_FROM_F30 27
#define KZGPOT_FP_F30_FROM_MONT1 28  /* f30_from_mont<1> */
#define KZGPOT_FP_F30_FROM_MONT2 29
#define KZGPOT_FP_MONT_FROM_F30_1 30 /* fp_mont_from_f30<1> */
#define KZGPOT_FP_MONT_FROM_F30_2 31
/* fp_subk_nr<KB> (a + KB - b) is KZGPOT_FP_SUBK + index, fp_negk_nr<KB> (KB - a) KZGPOT_FP_NEGK + index,
 * index = the constant's position in KZGPOT_FP_KB_LIST: every borrowed constant of
 * bls12_381_consts.hpp (csrc/ instantiates each of them); KB_EQ is the field's own (BN254 has no other) */
#define KZGPOT_FP_SUBK 32
#define KZGPOT_FP_NEGK 64
#define KZGPOT_FP_KB_LIST(X)                                                                                  \
  X(0, KB_2_28) X(1, KB_4_28) X(2, KB_8_28) X(3, KB_8_29) X(4, KB_16_28) X(5, KB_32_28) X(6, KB_32_29)        \
  X(7, KB_64_28) X(8, KB_64_29) X(9, KB_64_31) X(10, KB_128_28) X(11, KB_128_31) X(12, KB_4_29) X(13, KB_8_30) \
  X(14, KB_16_30) X(15, KB_64_30) X(16, KB_16_31) X(17, KB_EQ)
#define KZGPOT_FP_KB_COUNT 18
#define KZGPOT_FP_KB_EQ_INDEX 17
int kzgpot_test_fp_op(int op, int field, long n, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                      const uint32_t* d, const uint32_t* e, const uint32_t* f, uint32_t* r);
#ifdef __cplusplus
}
#endif
#endif
