"""The serial-chain forms of the radix-2^30 core (csrc/fp381.hpp f30_mul, f30_sqr, f30_mul_addsqr)
write a column's mads out by hand, a run of them to one asm statement. A product
that such a string drops, doubles or takes from the wrong digit shows in tests/test_gpu_f30_core.py
only as a wrong random digit; here every product slot is the ONLY non-zero product of some lane, so a
slip names its own slot (j, k):

  * f30_mul: a = sa 2^29 e_j, b = sb 2^29 e_k for all 13 x 13 ordered positions and the four sign
    pairs: lane (j, k) has the one product a_j b_k, in column j + k;
  * f30_sqr: all 91 operands s1 2^29 e_j + s2 2^29 e_k with j <= k (j = k: the single digit
    s1 2^29 e_j, which a squaring's digit bound allows; 2^30 it does not): the cross product
    a_j (2 a_k) and the two squares;
  * f30_mul_addsqr: the f30_mul cases with c = 0 (the product alone) and the f30_sqr cases as c with
    a = b = 0 (the squared operand alone).

Expected digits: the column-scan model of test_gpu_f30_core.py (tests/f30_ladder_model.py) on
Python integers, which raises where an int64 accumulator or an int32
digit would overflow, so every operand is also proven to be inside the device functions' range.
Launches: the hook of test_gpu_f30_core.py (libkzgpot_test.so kzgpot_test_f30_op), 256 lanes (one
block) and 320 lanes (a partial last block) at a time."""
import pytest

import f30_ladder_model as L
from test_gpu_f30_core import ARITY, LANES, MUL, MUL_ADDSQR, N, NAMES, SQR, expected, f30_op  # noqa: F401

D = 1 << 29
SIGNS = (1, -1)
ZERO = [0] * N


def _e(j, s):
    return [s * D if i == j else 0 for i in range(N)]


def _mul_cases():
    """(slot, operands): slot names the product a_j b_k"""
    return [((j, k, sa, sb), (_e(j, sa), _e(k, sb))) for j in range(N) for k in range(N) for sa in SIGNS for sb in SIGNS]


def _sqr_cases():
    out = []
    for j in range(N):
        for k in range(j, N):
            for s1 in SIGNS:
                for s2 in SIGNS if k > j else (s1,):
                    out.append(((j, k, s1, s2), ([a + b if k > j else a for a, b in zip(_e(j, s1), _e(k, s2))],)))
    return out


def _cases(op):
    if op == MUL:
        return _mul_cases()
    if op == SQR:
        return _sqr_cases()
    return ([(("a b",) + slot, (a, b, ZERO)) for slot, (a, b) in _mul_cases()]
            + [(("c^2",) + slot, (ZERO, ZERO, c)) for slot, (c,) in _sqr_cases()])


OPS = (MUL, SQR, MUL_ADDSQR)
_memo = {}


def cases(op):
    """(slots, operand tuples, expected digits), computed once per op"""
    if op not in _memo:
        cs = _cases(op)
        _memo[op] = ([s for s, _ in cs], [o for _, o in cs], [expected(op, o) for _, o in cs])
    return _memo[op]


def test_case_counts():
    assert len(cases(MUL)[0]) == 4 * 169
    assert len({(j, k) for j, k, _, _ in cases(SQR)[0]}) == 91 and len(cases(SQR)[0]) == 4 * 78 + 2 * 13
    assert len(cases(MUL_ADDSQR)[0]) == len(cases(MUL)[0]) + len(cases(SQR)[0])


@pytest.mark.parametrize("op", OPS, ids=[NAMES[o] for o in OPS])
def test_operands_inside_the_model(op):
    """the models accept every operand (no int64 / int32 overflow), and the expected digits are the
    right residues with balanced lower digits (needs no GPU)"""
    _, ops, want = cases(op)
    for o, r in zip(ops, want):
        v = [L.val(x) for x in o]
        num = v[0] * v[1] if op == MUL else v[0] * v[0] if op == SQR else v[0] * v[1] + v[2] * v[2]
        assert (L.val(r) * L.R30 - num) % L.P == 0
        assert all(-D <= d < D for d in r[:-1])


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("op", OPS, ids=[NAMES[o] for o in OPS])
def test_single_product_slots(f30_op, op, lanes):  # noqa: F811
    slots, ops, want = cases(op)
    assert len(ops[0]) == ARITY[op]
    bad = []
    for lo in range(0, len(ops), lanes):
        # every launch has `lanes` lanes: the last one is filled up from the front of the list
        idx = [(lo + t) % len(ops) for t in range(lanes)]
        got = f30_op(op, [ops[i] for i in idx])
        bad += [(i, g) for i, g in zip(idx, got) if g != want[i] and i >= lo]
    assert not bad, (f"{NAMES[op]}: {len(bad)} slots differ, first (j, k, signs) = {slots[bad[0][0]]}: "
                     f"got {bad[0][1]}, want {want[bad[0][0]]}; all: {sorted({slots[i][:-2] for i, _ in bad})[:40]}")
