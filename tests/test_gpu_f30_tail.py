"""The tail forms of the radix-2^30 scans (csrc/fp381.hpp f30_mul<K0, K1> / f30_sqr<K0, K1>) on the GPU,
one form per lane on supplied digits (libkzgpot_test.so kzgpot_test_f30_tail_op,
csrc/f30_tail_hooks.hip), against tests/f30_tail_model.py DIGIT FOR DIGIT, and the G1 subgroup ladders
that run them (csrc/curve.hpp jac<f30>) through k_g1_codec and k_g1_check<PairingBE> against the C
oracle.

Digit test, 4,096 lanes per form (16 blocks). The model raises if a 64-bit accumulator or a 32-bit
digit would overflow, so every operand set is also proven inside the device functions' range.
Operands (E = 2^29 + 4, the ladder states' digit bound; TOP = 2^23, their top-digit bound):
  * tail digits at their bound: every digit +E / -E / alternating, top digit +-TOP, for each tail;
  * the column sum at the model's worst case: product operands with every digit at +-E and the
    tails' signs chosen so that K t_k adds to the products' sign, both ways;
  * a carry across every digit boundary: a tail that is +-2^29 in ONE digit (+-TOP in the top one)
    and zero elsewhere, on random and on extreme products, for every digit, both signs and each tail,
    so that K t_k alone moves that column's carry (test_operands_reach_the_bounds counts the
    boundaries at which some lane's carry differs from the plain scan's: all twelve);
  * the top digit at its bound: the largest |value| of the products with the tails' top digits at
    +-TOP in the same direction;
  * zero tails (the plain scan's digits), and seeded random balanced values filling up the lanes.

Ladder test: 1,024 compressed / uncompressed G1 records drawn from tests/golden (subgroup points,
points of order 3 and 11 — the tripling's infinity and the equal-point branch of the first mixed
addition —, sums G + T, on-curve points off the subgroup, x with no square root, bad encodings):
bytes, per-point status and first_bad equal to the C oracle's."""
import ctypes
import random

import pytest

import f30_ladder_model as L
import f30_tail_model as T
from conftest import golden, oracle_run

N = 13
E = (1 << 29) + 4
TOP = 1 << 23
LANES = 4096
# KZGPOT_F30_TAIL_* (tests/kzgpot_test_f30_tail_hooks.h): (name, is a multiply, tail factors)
FORMS = {0: ("f30_mul<-1>", True, (-1,)), 1: ("f30_sqr<-2>", False, (-2,)), 2: ("f30_sqr<-1,-2>", False, (-1, -2)),
         3: ("f30_sqr<-1,-1>", False, (-1, -1)), 4: ("f30_mul<-16,64>", True, (-16, 64))}


def _alt(s, top=None):
    d = [s * E if k % 2 == 0 else -s * E for k in range(N)]
    return d if top is None else d[:-1] + [top]


def _unit(k, v):
    return [v if j == k else 0 for j in range(N)]


FULL = [[E] * (N - 1) + [TOP], [-E] * (N - 1) + [-TOP], _alt(1, TOP), _alt(-1, -TOP), [E] * (N - 1) + [-TOP],
        [-E] * (N - 1) + [TOP]]
ZERO = [0] * N


def _random(rng):
    return [rng.randrange(-(1 << 29), 1 << 29) for _ in range(N - 1)] + [rng.randrange(-TOP, TOP + 1)]


def operands(op, lanes=LANES):
    """lanes tuples (a, b, t0, t1); b / t1 None where the form takes none"""
    _, is_mul, ks = FORMS[op]
    rng = random.Random(4100 + op)
    out = []

    def add(a, b, ts):
        ts = list(ts) + [None] * (2 - len(ts))
        out.append((a, b if is_mul else None, ts[0], ts[1] if len(ks) == 2 else None))

    # tail digits at their bound, against extreme and random products; the worst-case column sums
    # (all terms of one sign: K t_k > 0 with a b > 0, K t_k < 0 with a b < 0) and the top digit's
    for a, b in ((FULL[0], FULL[0]), (FULL[0], FULL[1]), (FULL[2], FULL[2]), (FULL[2], FULL[3]), (FULL[1], FULL[1]),
                 (FULL[4], FULL[5]), (_random(rng), _random(rng))):
        for t in FULL:
            add(a, b, [t] * len(ks))
            add(a, b, [[-x if k < 0 else x for x in t] for k in ks])   # every K t_k of t's sign
            add(a, b, [[x if k < 0 else -x for x in t] for k in ks])   # ... and of the opposite sign
        add(a, b, [ZERO] * len(ks))
    # a carry across every digit boundary: one digit of one tail at +-2^29 (top: +-TOP)
    for j in range(len(ks)):
        for k in range(N):
            for s in (1, -1):
                t = _unit(k, s * (1 << 29) if k < N - 1 else s * TOP)
                for a, b in ((_random(rng), _random(rng)), (FULL[0], FULL[2])):
                    add(a, b, [t if i == j else ZERO for i in range(len(ks))])
    assert len(out) < lanes // 2
    while len(out) < lanes:
        add(_random(rng), _random(rng), [_random(rng) for _ in ks])
    return out


def expected(op, o):
    _, is_mul, ks = FORMS[op]
    a, b, t0, t1 = o
    tails = list(zip(ks, [t0, t1]))
    stats = {}
    r = T.scan([(a, b)], [], tails, stats) if is_mul else T.scan([], [a], tails, stats)
    return r, stats["peak"]


_cases = {}


def cases(op):
    """(operand tuples, expected digits, largest |column sum| of any lane), computed once per form"""
    if op not in _cases:
        ops = operands(op)
        exp = [expected(op, o) for o in ops]
        _cases[op] = (ops, [r for r, _ in exp], max(pk for _, pk in exp))
    return _cases[op]


@pytest.fixture(scope="module")
def tail_op(gpu):
    from kzgpot import _lib

    lib = ctypes.CDLL(_lib.TEST_LIB_PATH)
    fn = lib.kzgpot_test_f30_tail_op
    fn.restype = ctypes.c_int
    ptr = ctypes.POINTER(ctypes.c_int32)
    fn.argtypes = [ctypes.c_int, ctypes.c_long, ptr, ptr, ptr, ptr, ptr]

    def run(op, ops):
        n = len(ops)
        bufs = []
        for j in range(4):
            if ops[0][j] is None:
                bufs.append(None)
            else:
                bufs.append((ctypes.c_int32 * (N * n))(*[x for o in ops for x in o[j]]))
        out = (ctypes.c_int32 * (N * n))()
        rc = fn(op, n, *bufs, out)
        assert rc == 0, rc
        return [list(out[N * i:N * i + N]) for i in range(n)]

    return run


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(FORMS), ids=[FORMS[o][0] for o in sorted(FORMS)])
def test_digits_exact(tail_op, op):
    ops, want, _ = cases(op)
    got = tail_op(op, ops)
    bad = [i for i in range(len(ops)) if got[i] != want[i]]
    assert not bad, f"{FORMS[op][0]}: lane {bad[0]} of {len(bad)} differs: operands {ops[bad[0]]}, got {got[bad[0]]}, want {want[bad[0]]}"


@pytest.mark.parametrize("op", sorted(FORMS), ids=[FORMS[o][0] for o in sorted(FORMS)])
def test_operands_reach_the_bounds(op):
    """what the lanes are for (needs no GPU): the expected digits are the right integers, balanced;
    a lane's tail changes a carry at every digit boundary; the all-extreme lanes' column sums pass
    2^61 (13 products of 2^58 and the m p terms, whose signs the operands do not choose; the calculus
    allows 2^62.8), and their top digit comes within a carry of sum |K| TOP"""
    name, is_mul, ks = FORMS[op]
    ops, want, peak = cases(op)
    assert len(ops) == LANES
    crossed, top_seen = set(), 0
    for (a, b, t0, t1), r in zip(ops, want):
        ts = [t for t in (t0, t1) if t is not None]
        plain = L._scan([(a, b)], []) if is_mul else L._scan([], [a])
        assert L.val(r) == L.val(plain) + sum(k * L.val(t) for k, t in zip(ks, ts))
        assert all(-(1 << 29) <= d < (1 << 29) for d in r[:-1])
        top_seen = max(top_seen, abs(r[-1]))
        # digit k's carry out differs from the plain scan's: the boundary between digits k and k + 1
        lin = [sum(k * t[i] for k, t in zip(ks, ts)) for i in range(N)]
        c = 0
        for i in range(N - 1):
            s = plain[i] + lin[i] + c
            c = (s + (1 << 29)) >> 30
            if c:
                crossed.add(i)
    assert crossed == set(range(N - 1))
    st = L.B(E, TOP, (E * L.LOW) + (TOP << 360))
    bound = T.product_tail([(L.bound_only(st),) * 2] if is_mul else [], [] if is_mul else [L.bound_only(st)],
                           [(k, L.bound_only(st)) for k in ks], name)
    assert (1 << 61) < peak <= bound.worst
    assert sum(abs(k) for k in ks) * TOP - (1 << 21) <= top_seen <= bound.b.top


# ------------------------------------------------------------------------------- the ladders
def _stream(vecs, n, seed):
    rng = random.Random(seed)
    recs = [bytes.fromhex(v["in"]) for v in vecs]
    return b"".join(recs + [rng.choice(recs) for _ in range(n - len(recs))])


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["g1_decompress", "g1_transcode"], ids=["k_g1_codec", "k_g1_check-PairingBE"])
def test_ladders_against_the_c_oracle(gpu, oracle_lib, op):
    n = 1024
    vecs = golden(op)
    notes = " ".join(v["note"] for v in vecs)
    assert "order-3 point" in notes and "order-11 point" in notes and "subgroup point" in notes
    data = _stream(vecs, n, 4200)
    got = gpu.run_codec(op, data, 0, want_status=True)
    out, st, fb, ret = oracle_run(oracle_lib, op, data, n)
    assert got.status == st
    assert got.out == out
    assert got.first_bad == fb
    assert 0 in set(st) and 5 in set(st)  # accepted points, and points rejected by the subgroup test
