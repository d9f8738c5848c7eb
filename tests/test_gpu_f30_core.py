"""The radix-2^30 field core's functions (csrc/fp381.hpp f30_mul, f30_sqr, f30_mul_addsqr,
f30_mul_sum2, f30_dbl, f30_mul3, f30_norm<S>) on the GPU, one function per lane on supplied digits
(libkzgpot_test.so kzgpot_test_f30_op, csrc/f30_hooks.hip), against exact Python integers DIGIT FOR
DIGIT: the codec tests see canonical bytes only and cannot steer an internal digit to the edge of a
bound, and a rewrite of how a digit is computed (a doubling as an add, an unbiased upper-column digit,
one serial mad chain per column) must leave every output digit the same integer.

Expected digits: the column scan and f30_norm of tests/f30_ladder_model.py (the one model of the
core; tests/test_fp30.py drives the same scan), which compute the column sums, m_i and
carries on Python integers and raise if a 64-bit accumulator or a 32-bit digit would overflow — so
every operand set below is also proven to be inside the device functions' range.

Operands (E = 2^29 + 4, f30_norm's slack over a balanced digit):
  * every digit +E, every digit -E, alternating signs both ways (all 13 digits);
  * top digit +-2^23 with the lower digits extreme (the products' stated operand bound);
  * one operand digit-wise doubled (digits 2^30 + 8, top 2^24) where the function allows it:
    f30_mul's first operand and f30_norm<S> (f30_sqr, the two-product forms, f30_dbl and f30_mul3
    would leave int64 / int32 there, as the model confirms in test_doubled_operand_limits);
  * zero, and +-1 in a single digit (bottom, middle, top);
  * seeded random balanced values filling up the lanes.
Run on 256 lanes (one block) and 320 lanes (a partial last block)."""
import ctypes
import random

import pytest

import f30_ladder_model as L

N = 13
E = (1 << 29) + 4
TOP = 1 << 23
LANES = [256, 320]
# KZGPOT_F30_* (tests/kzgpot_test_f30_hooks.h)
MUL, SQR, MUL_ADDSQR, MUL_SUM2, DBL, MUL3, NORM0, NORM1, NORM2, NORM3 = range(10)
ARITY = {MUL: 2, SQR: 1, MUL_ADDSQR: 3, MUL_SUM2: 4, DBL: 1, MUL3: 1, NORM0: 1, NORM1: 1, NORM2: 1, NORM3: 1}
NAMES = {MUL: "f30_mul", SQR: "f30_sqr", MUL_ADDSQR: "f30_mul_addsqr", MUL_SUM2: "f30_mul_sum2", DBL: "f30_dbl",
         MUL3: "f30_mul3", NORM0: "f30_norm<0>", NORM1: "f30_norm<1>", NORM2: "f30_norm<2>", NORM3: "f30_norm<3>"}


def _alt(s):
    return [s * E if k % 2 == 0 else -s * E for k in range(N)]


def _unit(k, s):
    return [s if j == k else 0 for j in range(N)]


FULL = [[E] * N, [-E] * N, _alt(1), _alt(-1)]
TOPPED = [[E] * (N - 1) + [TOP], [-E] * (N - 1) + [-TOP], _alt(1)[:-1] + [TOP], [E] * (N - 1) + [-TOP],
          _alt(-1)[:-1] + [-TOP], [-E] * (N - 1) + [TOP]]
SMALL = [[0] * N] + [_unit(k, s) for k in (0, 6, 12) for s in (1, -1)]
DOUBLED = [[2 * x for x in d] for d in TOPPED]
EDGES = FULL + TOPPED + SMALL


def _random(rng):
    return [rng.randrange(-(1 << 29), 1 << 29) for _ in range(N - 1)] + [rng.randrange(-TOP, TOP + 1)]


def _s32(x):
    assert -(1 << 31) <= x < (1 << 31), "the operand leaves int32 in a digit-wise form"
    return x


def _norm(a, s):
    b = L.B(max(abs(x) for x in a[:-1]), abs(a[-1]), abs(L.val(a)))
    return L.norm(L.V(a, b), s).d


def expected(op, ops):
    a = ops[0]
    if op == MUL:
        return L._scan([(a, ops[1])], [])
    if op == SQR:
        return L._scan([], [a])
    if op == MUL_ADDSQR:
        return L._scan([(a, ops[1])], [ops[2]])
    if op == MUL_SUM2:
        return L._scan([(a, ops[1]), (ops[2], ops[3])], [])
    if op == DBL:
        return [_s32(2 * x) for x in a]
    if op == MUL3:
        return [_s32(3 * x) for x in a]
    return _norm(a, op - NORM0)


def operands(op, lanes):
    """lanes operand tuples for op: the edge patterns first (every pattern as the first operand, the
    others rotated against it so that equal and opposite signs both meet), then seeded random ones"""
    k = ARITY[op]
    if op in (NORM2, NORM3):
        first = TOPPED + SMALL + DOUBLED  # 2^S x a top digit of E would leave int32
    else:
        first = EDGES + (DOUBLED if op in (MUL, NORM0, NORM1) else [])
    out = []
    for t, a in enumerate(first):
        others = TOPPED + SMALL if a in DOUBLED else EDGES  # a doubled operand meets the stated bound only
        out.append(tuple([a] + [others[(t + 3 * j) % len(others)] for j in range(1, k)]))
    if k > 1:
        # all operands at the same extreme, and products of opposite signs: the largest column sums
        for a, b in ((FULL[0], FULL[0]), (FULL[0], FULL[1]), (TOPPED[0], TOPPED[0]), (TOPPED[0], TOPPED[1]),
                     (FULL[2], FULL[2]), (FULL[2], FULL[3])):
            out.append(tuple([a, b, a, b][:k]))
    rng = random.Random(3000 + op)
    assert len(out) < 64
    while len(out) < lanes:
        out.append(tuple(_random(rng) for _ in range(k)))
    return out


_cases = {}


def cases(op):
    """(operand tuples, expected digits) for max(LANES) lanes, computed once per op"""
    if op not in _cases:
        ops = operands(op, max(LANES))
        _cases[op] = (ops, [expected(op, o) for o in ops])
    return _cases[op]


@pytest.fixture(scope="module")
def f30_op(gpu):
    from kzgpot import _lib

    lib = ctypes.CDLL(_lib.TEST_LIB_PATH)
    fn = lib.kzgpot_test_f30_op
    fn.restype = ctypes.c_int
    ptr = ctypes.POINTER(ctypes.c_int32)
    fn.argtypes = [ctypes.c_int, ctypes.c_long, ptr, ptr, ptr, ptr, ptr]

    def run(op, ops):
        n = len(ops)
        bufs = []
        for j in range(4):
            if j < ARITY[op]:
                flat = [x for o in ops for x in o[j]]
                bufs.append((ctypes.c_int32 * (N * n))(*flat))
            else:
                bufs.append(None)
        out = (ctypes.c_int32 * (N * n))()
        rc = fn(op, n, *bufs, out)
        assert rc == 0, rc
        return [list(out[N * i:N * i + N]) for i in range(n)]

    return run


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("op", sorted(NAMES), ids=[NAMES[o] for o in sorted(NAMES)])
def test_digits_exact(f30_op, op, lanes):
    ops, want = cases(op)
    got = f30_op(op, ops[:lanes])
    bad = [i for i in range(lanes) if got[i] != want[i]]
    assert not bad, f"{NAMES[op]}: lane {bad[0]} of {len(bad)} differs: operands {ops[bad[0]]}, got {got[bad[0]]}, want {want[bad[0]]}"


@pytest.mark.parametrize("op", sorted(NAMES), ids=[NAMES[o] for o in sorted(NAMES)])
def test_operands_inside_the_model(op):
    """every operand set passes the models' int64 / int32 checks, and the products are the right
    residues with balanced lower digits (needs no GPU)"""
    ops, want = cases(op)
    assert len(ops) == max(LANES)
    for o, r in zip(ops, want):
        v = [L.val(x) for x in o]
        if op in (MUL, SQR, MUL_ADDSQR, MUL_SUM2):
            num = {MUL: lambda: v[0] * v[1], SQR: lambda: v[0] * v[0], MUL_ADDSQR: lambda: v[0] * v[1] + v[2] * v[2],
                   MUL_SUM2: lambda: v[0] * v[1] + v[2] * v[3]}[op]()
            assert (L.val(r) * L.R30 - num) % L.P == 0
            assert all(-(1 << 29) <= d < (1 << 29) for d in r[:-1])
        else:
            scale = {DBL: 2, MUL3: 3, NORM0: 1, NORM1: 2, NORM2: 4, NORM3: 8}[op]
            assert L.val(r) == scale * v[0]


def test_doubled_operand_limits():
    """why only f30_mul's first operand and f30_norm take a digit-wise doubled value here"""
    d, b = DOUBLED[0], TOPPED[0]
    for f in (lambda: L._scan([], [d]), lambda: L._scan([(d, b), (b, b)], []), lambda: L._scan([(d, b)], [b]),
              lambda: [_s32(2 * x) for x in d], lambda: [_s32(3 * x) for x in d]):
        with pytest.raises((OverflowError, AssertionError)):
            f()
    L._scan([(d, b)], [])
