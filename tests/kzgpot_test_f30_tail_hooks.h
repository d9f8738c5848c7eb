/*
 * Test-only entry point of libkzgpot_test.so (kzg-setup-powersoftau_amd/Makefile, built with
 * -DKZGPOT_TEST_HOOKS) for the TAIL forms of the radix-2^30 scans, beside
 * tests/kzgpot_test_f30_hooks.h. The product library (libkzgpot.so) exports none of this.
 */
#ifndef KZGPOT_TEST_F30_TAIL_HOOKS_H
#define KZGPOT_TEST_F30_TAIL_HOOKS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* One tail form (csrc/fp381.hpp f30_mul<K0, K1> / f30_sqr<K0, K1>) per GPU lane, on host arrays of
 * 13 int32 digits per lane (lane i at [13 i, 13 i + 13)), in blocks of 256 lanes
 * (csrc/f30_tail_hooks.hip): r = the balanced digits of a b 2^-390 (SQR: a^2 2^-390; b may be NULL)
 * + K0 t0 + K1 t1, with (K0, K1) the form's factors; a form with one tail takes t1 = NULL.
 *   the ladders' forms: MUL_M1 (-1) H and r of the mixed addition, SQR_M2 (-2) the doubling's X3,
 *   SQR_M1_M2 (-1, -2) the mixed addition's X3, SQR_M1_M1 (-1, -1) the tripling's U;
 *   the ends of the factor range: MUL_M16_64 (-16, 64).
 * The digits are whatever the caller supplies: keeping them inside the functions' stated operand
 * bounds is the caller's business. Returns 0 or a negative KZGPOT_E_*. */
#define KZGPOT_F30_TAIL_MUL_M1 0
#define KZGPOT_F30_TAIL_SQR_M2 1
#define KZGPOT_F30_TAIL_SQR_M1_M2 2
#define KZGPOT_F30_TAIL_SQR_M1_M1 3
#define KZGPOT_F30_TAIL_MUL_M16_64 4
int kzgpot_test_f30_tail_op(int op, long n, const int32_t* a, const int32_t* b, const int32_t* t0, const int32_t* t1,
                            int32_t* r);
#ifdef __cplusplus
}
#endif
#endif
