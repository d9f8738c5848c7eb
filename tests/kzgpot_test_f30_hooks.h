/*
 * Test-only entry point of libkzgpot_test.so (kzg-setup-powersoftau_amd/Makefile, built with
 * -DKZGPOT_TEST_HOOKS) for the radix-2^30 field core, beside those of tests/kzgpot_test_hooks.h.
 * The product library (libkzgpot.so) exports none of this.
 */
#ifndef KZGPOT_TEST_F30_HOOKS_H
#define KZGPOT_TEST_F30_HOOKS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* One function of the radix-2^30 field core (csrc/fp381.hpp f30_*) per GPU lane, on host arrays of
 * 13 int32 digits per lane (lane i at [13 i, 13 i + 13)), in blocks of 256 lanes
 * (csrc/f30_hooks.hip): r = op(a[, b[, c[, d]]]); operands an op does not take may be NULL.
 *   MUL a b, SQR a^2, MUL_ADDSQR a b + c^2, MUL_SUM2 a b + c d (all times 2^-390 mod p);
 *   DBL 2a and MUL3 3a digit-wise; NORM<S> f30_norm<S>(a) = 2^S a renormalised.
 * The digits are whatever the caller supplies: keeping them inside the functions' stated operand
 * bounds is the caller's business. Returns 0 or a negative KZGPOT_E_*. */
#define KZGPOT_F30_MUL 0
#define KZGPOT_F30_SQR 1
#define KZGPOT_F30_MUL_ADDSQR 2
#define KZGPOT_F30_MUL_SUM2 3
#define KZGPOT_F30_DBL 4
#define KZGPOT_F30_MUL3 5
#define KZGPOT_F30_NORM0 6
#define KZGPOT_F30_NORM1 7
#define KZGPOT_F30_NORM2 8
#define KZGPOT_F30_NORM3 9
int kzgpot_test_f30_op(int op, long n, const int32_t* a, const int32_t* b, const int32_t* c, const int32_t* d,
                       int32_t* r);
#ifdef __cplusplus
}
#endif
#endif
