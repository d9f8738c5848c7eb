/*
 * Test-only entry point of libkzgpot_test.so (kzg-setup-powersoftau_amd/Makefile, built with
 * -DKZGPOT_TEST_HOOKS) for the pairing product's device functions on cells (csrc/pairing_parts.hpp),
 * beside tests/kzgpot_test_fp_hooks.h. The product library (libkzgpot.so) exports none of this.
 */
#ifndef KZGPOT_TEST_PAIRING_HOOKS_H
#define KZGPOT_TEST_PAIRING_HOOKS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* One function of pairing_parts.hpp per GPU lane, in blocks of 64 lanes as k_pair_miller runs them
 * (csrc/pairing_hooks.hip), on the caller's cells.
 *
 * cells: the kernels' own layout, KZGPOT_PAIR_CELLS cells of one Fq2 (28 words: c0's 14 limbs, c1's 14)
 * per lane, word-major: word w of cell c of lane i at cells[(28 c + w) stride + i]. stride >= lanes > 0
 * and at most KZGPOT_PAIR_MAX_STRIDE (the product call's stride is a multiple of 64; the functions do not
 * depend on that, and the test also runs a stride that is none). The limbs are Montgomery and taken as
 * supplied: keeping them "reduced" (limbs < 2^28, value < 2 p) is the caller's business. The entry copies
 * all of `cells` to the device, runs `op` once in each lane < lanes, and copies everything back in place:
 * the caller sees every cell of every lane, the lanes >= lanes included.
 *
 * arg[0..3]: the function's cell arguments in its own order, then its integer argument; arguments an op
 * does not take are ignored. Every cell range an op touches must lie inside the lane's cells, which the
 * entry checks; that a destination does not overlap an operand where the function forbids it is the
 * caller's business (pairing_parts.hpp states it per function).
 *
 *   op                  arg[0], arg[1], arg[2]; arg[3]        cells per argument
 *   C_MUL C_ADD C_SUB   d, a, b                                1
 *   C_SQR C_NEG C_MUL_XI C_HALF C_INV   d, a                   1
 *   C_MUL_FQ            d, a, s; which (0 or 1)                1
 *   X_MUL6 / X_MUL3     d, a, b  (x_mul, n = 6 / 3, product)   6 / 3
 *   X_SQR6 / X_SQR3     d, a     (x_mul, n = 6 / 3, square)    6 / 3
 *   X_MUL_LINE          d, a, l                                6, 6, 3
 *   X_FROB              d, a; k (1 or 2)                       6
 *   X_CONJ              d, a                                   6
 *   X6_INV              d, a, s                                3, 3, 5
 *   X12_INV             d, a, s                                6, 6, 17
 *   X12_POW_X           d, a  (and the cells T = 30 .. 35)     6
 *   MILLER_DOUBLE, MILLER_ADD   none: the Miller kernel's cell layout (F = 0 .. S7 = 28)
 *   TREE                none: the product of the F cells (0 .. 5) of lanes 0 .. count - 1 into lane 0's,
 *                       through launch_pair_tree, the level loop of the product call; 1 <= count <= lanes.
 *                       It writes F and G (6 .. 11) of the lanes that multiply.
 * Returns 0 or a negative KZGPOT_E_*. */
#define KZGPOT_PAIR_CELLS 56 /* kPairFinalCells (csrc/plans.hpp) */
#define KZGPOT_PAIR_CELL_WORDS 28
#define KZGPOT_PAIR_MAX_STRIDE 4096

#define KZGPOT_PAIR_C_MUL 0
#define KZGPOT_PAIR_C_SQR 1
#define KZGPOT_PAIR_C_ADD 2
#define KZGPOT_PAIR_C_SUB 3
#define KZGPOT_PAIR_C_NEG 4
#define KZGPOT_PAIR_C_MUL_XI 5
#define KZGPOT_PAIR_C_HALF 6
#define KZGPOT_PAIR_C_MUL_FQ 7
#define KZGPOT_PAIR_C_INV 8
#define KZGPOT_PAIR_X_MUL6 9
#define KZGPOT_PAIR_X_SQR6 10
#define KZGPOT_PAIR_X_MUL3 11
#define KZGPOT_PAIR_X_SQR3 12
#define KZGPOT_PAIR_X_MUL_LINE 13
#define KZGPOT_PAIR_X_FROB 14
#define KZGPOT_PAIR_X_CONJ 15
#define KZGPOT_PAIR_X6_INV 16
#define KZGPOT_PAIR_X12_INV 17
#define KZGPOT_PAIR_X12_POW_X 18
#define KZGPOT_PAIR_MILLER_DOUBLE 19
#define KZGPOT_PAIR_MILLER_ADD 20
#define KZGPOT_PAIR_TREE 21
#define KZGPOT_PAIR_OP_COUNT 22
int kzgpot_test_pairing_op(int op, const int32_t arg[4], long lanes, long stride, long count, uint32_t* cells);
#ifdef __cplusplus
}
#endif
#endif
