"""The 14 x 28 / 9 x 29 limb core of csrc/fp381.hpp on the GPU, one function per lane on supplied limbs
(libkzgpot_test.so kzgpot_test_fp_op, csrc/fp_hooks.hip; tests/kzgpot_test_fp_hooks.h), against the exact
integer model tests/fp28_model.py LIMB FOR LIMB: the five multiply forms, the reductions and comparisons,
fp_is_zero / fp_eq / f30_is_zero<F30_ZK>, every borrowed-constant form fp_subk_nr<K> / fp_negk_nr<K>, the
word and Montgomery conversions, the Fp2 f_mul / f_sqr and the 14 x 28 <-> 13 x 30 conversions, for
BLS12-381 and, where bn254_kernels.hip uses a function, BN254. The codec tests see canonical bytes only:
they never hand a multiply a limb above 2^28, a zero test a nonzero value that passes its filter (2^-20
of random values), or a borrowed constant a limb at its dominance bound.

A hook kernel inlines the functions in its own context, not in the codecs' register pressure or under
their scheduler flags: like the radix-2^30 hook (tests/test_gpu_f30_core.py) this pins what the SOURCE
means under hipcc — every output limb the integer the model computes — not the codecs' instruction streams.

Every operand set goes through the model first, which raises where a uint64 accumulator, a 32-bit limb, a
signed borrow chain or the result's NL limbs would overflow, so nothing reaches the device outside the
functions' stated ranges (test_operands_inside_the_model, no GPU).

Multiply forms, per form:
  * one lane for every distinct operand-bound tuple the interval proof records (field_bounds_model.RECORD,
    driven through the entry points of test_field_bounds.py, test_field_bounds_msm.py and
    test_field_bounds_lagrange.py, and the BN254 chain), EVERY LIMB AT ITS BOUND; none is left out;
  * limb-bit classes at the limit: fp_mul's documented limb-bit sums of 60 (28 + 32 with limbs up to
    2^32 - 17, 29 + 31, 30 + 30, both orders); the k-product forms at the sums for which k 14 2^s + 14 2^56
    stays below 2^64 (59 for fp_mul_sum2 and fp_mul_add8sqr, 58 for fp_mul_sum3); fp_sqr at 30 bits, and
    with one limb at 2^31 - 1 (its doubling's edge; all limbs there leave uint64, as the model confirms in
    test_sqr_limit). Lower limbs at the class maximum, the top limbs the largest for which the model's
    result still fits (a search on the CPU model);
  * zero, a single 1 (bottom, middle, top limb), p, p - 1 and R mod p as limbs; seeded random filler.
Zero tests: 64-lane groups composed as waves (no candidate, all zeros, interleaved, one zero in lane 0 /
lane 63, nonzero values k p + d that pass the filter), zeros k p for every k the precondition allows in
normalized form, with a carry left in a limb, and (k <= the constant's multiple) as KB_EQ - b.
f30_is_zero<16>: the same plan over k in [-16, 16] with balanced digits, a digit +- 2^30 or +- 2^31 against
its neighbour (magnitudes up to 2^31 - 2^29: a multiple of p fixes every digit mod 2^30, so a zero cannot
hold an arbitrary digit), and digits at exactly +-(2^31 - 1) in the nonzero lanes.
Each op runs on its first 256 lanes and on all of them, a count that leaves a partial last wave."""
import ctypes
import inspect
import random

import pytest

import f30_ladder_model as L
import field_bounds_model as M
import fp28_model as F28
from fp28_model import BLS, BN254, U32

CAP = (1 << 32) - 17  # the largest limb fp_norm / fp_canon / fp_is_zero take (limbs < 2^32 - 16)
MIN_LANES = 357       # 320 + 37: five full waves and a partial one
KB_NAMES = ["KB_2_28", "KB_4_28", "KB_8_28", "KB_8_29", "KB_16_28", "KB_32_28", "KB_32_29", "KB_64_28", "KB_64_29",
            "KB_64_31", "KB_128_28", "KB_128_31", "KB_4_29", "KB_8_30", "KB_16_30", "KB_64_30", "KB_16_31", "KB_EQ"]
BOTH = ("bls12_381", "bn254")
BLS_ONLY = ("bls12_381",)


def _s32(x):
    return x - (1 << 32) if x >> 31 else x


def _u(d):
    return [x & U32 for x in d]


# name -> (code, arity, fields, operand width, result width, model(F, *operands) -> result words);
# widths: L = NL limbs, W = NW words, D = 13 digits (int32 as their 32 bits), P = one predicate word
OPS = {
    "fp_mul": (0, 2, BOTH, "L", "L", F28.mul),
    "fp_sqr": (1, 1, BOTH, "L", "L", F28.sqr),
    "fp_mul_sum2": (2, 4, BLS_ONLY, "L", "L", F28.mul_sum2),
    "fp_mul_sum3": (3, 6, BLS_ONLY, "L", "L", F28.mul_sum3),
    "fp_mul_addsqr<8>": (5, 3, BLS_ONLY, "L", "L", F28.mul_add8sqr),  # fp_mul_add8sqr, under the id it has had
    "fp_norm": (6, 1, BLS_ONLY, "L", "L", F28.norm),
    "fp_half": (7, 1, BLS_ONLY, "L", "L", F28.half),
    "fp_reduce_once": (8, 1, BLS_ONLY, "L", "L", F28.reduce_once),
    "fp_reduce_canon": (9, 1, BLS_ONLY, "L", "L", F28.reduce_canon),
    "fp_canon": (10, 1, BLS_ONLY, "L", "L", F28.canon),
    "fp_is_zero": (11, 1, BOTH, "L", "P", lambda F, a: [int(F28.is_zero(F, a))]),
    "fp_eq": (12, 2, BOTH, "L", "P", lambda F, a, b: [int(F28.eq(F, a, b))]),
    "fp_lt_canon": (13, 2, BOTH, "L", "P", lambda F, a, b: [int(F28.lt_canon(F, a, b))]),
    "fp_neg_canon": (14, 1, BOTH, "L", "L", F28.neg_canon),
    "fp_cond_sub_2p": (15, 1, BLS_ONLY, "L", "L", F28.cond_sub_2p),
    "fp_add_red": (16, 2, BLS_ONLY, "L", "L", F28.add_red),
    "fp_sub_red": (17, 2, BLS_ONLY, "L", "L", F28.sub_red),
    "f_mul(fp2)": (18, 4, BLS_ONLY, "L", "LL", lambda F, *o: [x for c in F28.f2_mul(F, *o) for x in c]),
    "f_sqr(fp2)": (19, 2, BLS_ONLY, "L", "LL", lambda F, *o: [x for c in F28.f2_sqr(F, *o) for x in c]),
    "fp_from_words": (20, 1, BOTH, "W", "L", F28.from_words),
    "fp_to_words": (21, 1, BOTH, "L", "W", F28.to_words),
    "fp_to_mont": (22, 1, BOTH, "L", "L", F28.to_mont),
    "fp_from_mont": (23, 1, BOTH, "L", "L", F28.from_mont),
    "fp_add": (24, 2, BOTH, "L", "L", F28.add),
    "f30_is_zero<16>": (25, 1, BLS_ONLY, "D", "P", lambda F, z: [int(F28.f30_is_zero([_s32(x) for x in z]))]),
    "f30_from_fp": (26, 1, BLS_ONLY, "L", "D", lambda F, a: _u(F28.f30_from_fp(a))),
    "fp_from_f30": (27, 1, BLS_ONLY, "D", "L", lambda F, z: F28.fp_from_f30([_s32(x) for x in z])),
    "f30_from_mont<1>": (28, 1, BLS_ONLY, "L", "D", lambda F, a: _u(F28.f30_from_mont(1, a))),
    "f30_from_mont<2>": (29, 1, BLS_ONLY, "L", "D", lambda F, a: _u(F28.f30_from_mont(2, a))),
    "fp_mont_from_f30<1>": (30, 1, BLS_ONLY, "D", "L", lambda F, z: F28.fp_mont_from_f30(1, [_s32(x) for x in z])),
    "fp_mont_from_f30<2>": (31, 1, BLS_ONLY, "D", "L", lambda F, z: F28.fp_mont_from_f30(2, [_s32(x) for x in z])),
}
for _i, _k in enumerate(KB_NAMES):
    _f = BOTH if _k == "KB_EQ" else BLS_ONLY
    OPS[f"fp_subk_nr<{_k}>"] = (32 + _i, 2, _f, "L", "L", lambda F, a, b, k=_k: F28.subk(F, k, a, b))
    OPS[f"fp_negk_nr<{_k}>"] = (64 + _i, 1, _f, "L", "L", lambda F, b, k=_k: F28.negk(F, k, b))
assert L.ZK == 16 and KB_NAMES == list(BLS.KB)  # curve.hpp F30_ZK; the header's borrowed constants, in its order

MUL_FORMS = {  # op -> (recorded form, numerator of the residue)
    "fp_mul": ("mul", lambda v: v[0] * v[1]),
    "fp_sqr": ("sqr", lambda v: v[0] * v[0]),
    "fp_mul_sum2": ("mul_sum2", lambda v: v[0] * v[1] + v[2] * v[3]),
    "fp_mul_sum3": ("mul_sum3", lambda v: v[0] * v[1] + v[2] * v[3] + v[4] * v[5]),
    "fp_mul_addsqr<8>": ("mul_add8sqr", lambda v: v[0] * v[1] + 8 * v[2] * v[2]),
}
# limb-bit classes per operand (see the module docstring)
CLASSES = {
    "fp_mul": [(28, 32), (32, 28), (29, 31), (31, 29), (30, 30)],
    "fp_sqr": [(30,)],
    "fp_mul_sum2": [(x, y, x, y) for x, y in ((28, 31), (31, 28), (29, 30), (30, 29))] + [(28, 31, 31, 28), (29, 30, 30, 29)],
    "fp_mul_sum3": [(x, y) * 3 for x, y in ((28, 30), (30, 28), (29, 29))] + [(28, 30, 30, 28, 29, 29)],
    "fp_mul_addsqr<8>": [(x, y, 28) for x, y in ((28, 31), (31, 28), (29, 30), (30, 29))],
}


def _cls_max(bits):
    return CAP if bits == 32 else (1 << bits) - 1


# ------------------------------------------------------------------------------- the recorded sites
_recorded = None


def recorded():
    """(field, form) -> sorted distinct operand-bound tuples, from one recorded run of the interval proofs'
    entry points (the parameterless tests of the three files but the deliberate overflow, and the BN254
    chain under use_field("bn254")); the recorder is off and the field is BLS12-381 again afterwards"""
    global _recorded
    if _recorded is None:
        import test_field_bounds as A
        import test_field_bounds_lagrange as C
        import test_field_bounds_msm as B

        assert M.RECORD is None
        M.RECORD = rec = {}
        try:
            for mod in (A, B, C):
                for name, fn in sorted(vars(mod).items()):
                    if (name.startswith("test_") and inspect.isfunction(fn) and fn.__module__ == mod.__name__
                            and name != "test_bounds_model_catches_overflow" and not inspect.signature(fn).parameters):
                        fn()
            M.use_field("bn254")
            try:
                A.test_bn254_decompress_chain(M)
            finally:
                M.use_field("bls12_381")
        finally:
            M.RECORD = None
        out = {}
        for (field, form, _), tuples in rec.items():
            out.setdefault((field, form), set()).update(tuples)
        _recorded = {k: sorted(v) for k, v in out.items()}
    return _recorded


# ------------------------------------------------------------------------------- representations
def loosen(F, limbs, cap=CAP):
    """the same value with as much as fits moved DOWN into each limb (limbs up to cap)"""
    r = list(limbs)
    for i in range(F.NL - 2, -1, -1):
        e = max(0, min(r[i + 1], (cap - r[i]) >> F.LB))
        r[i] += e << F.LB
        r[i + 1] -= e
    assert F.val(r) == F.val(limbs) and all(x <= max(cap, y) for x, y in zip(r, limbs))
    return r


def carry_left(F, limbs, j):
    """the same value with a carry left in limb j: limb j + 2^LB, limb j+1 - 1 (None if limb j+1 is 0)"""
    if limbs[j + 1] == 0:
        return None
    r = list(limbs)
    r[j] += 1 << F.LB
    r[j + 1] -= 1
    return r


def dominated(F, K, v):
    """limbs of v with limb i <= K[i], taken greedily from the top (None if v does not fit under K)"""
    r = [0] * F.NL
    for i in range(F.NL - 1, -1, -1):
        r[i] = min(K[i], v >> (F.LB * i))
        v -= r[i] << (F.LB * i)
    return r if v == 0 else None


def _unit(F, k):
    return [int(j == k) for j in range(F.NL)]


def small(F):
    return [[0] * F.NL, _unit(F, 0), _unit(F, F.NL // 2), _unit(F, F.NL - 1), F.limbs(F.p), F.limbs(F.p - 1), F.C["ONE"]]


def rnd(F, rng, vmax):
    return F.limbs(rng.randrange(vmax))


# ------------------------------------------------------------------------------- multiply forms
def _accepts(F, op, ops):
    try:
        OPS[op][5](F, *ops)
        return True
    except (OverflowError, AssertionError):
        return False


def _largest(ok, hi):
    """the largest t in [0, hi] with ok(t), ok monotone and ok(0) true"""
    assert ok(0)
    if ok(hi):
        return hi
    lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


def class_lanes(F, op):
    out = []
    n = F.NL
    for cls in CLASSES[op]:
        lows = [_cls_max(b) for b in cls]

        def build(tops):
            return tuple([lo] * (n - 1) + [min(t, lo)] for lo, t in zip(lows, tops))

        # a common top limb, then each operand's own pushed as far as the others (at 0) leave room
        t = _largest(lambda t: _accepts(F, op, build([t] * len(lows))), max(lows))
        out.append(build([t] * len(lows)))
        for k in range(len(lows)):
            tk = _largest(lambda t: _accepts(F, op, build([t if j == k else 0 for j in range(len(lows))])), lows[k])
            out.append(build([tk if j == k else 0 for j in range(len(lows))]))
    if op == "fp_sqr":  # one limb at 2^31 - 1, where 2 a_k just fits 32 bits
        for k in (0, n // 2, n - 2):
            def one(u, t):
                a = [u] * (n - 1) + [t]
                a[k] = (1 << 31) - 1
                return (a,)
            u = _largest(lambda u: _accepts(F, op, one(u, 0)), (1 << 30) - 1)
            t = _largest(lambda t: _accepts(F, op, one(u, t)), u)
            out += [one(u, t), one(u, 0)]
    if op.startswith("fp_mul_addsqr"):  # the squared operand's doubling / scaling edge: 2 S c_k at 32 bits
        cmax = ((1 << 32) - 1) // (2 * 8)
        for k in (0, n // 2, n - 2):
            c = [F.MASK] * (n - 1) + [0]
            c[k] = cmax
            u = _largest(lambda u: _accepts(F, op, ([u] * (n - 1) + [0], [u] * (n - 1) + [0], c)), (1 << 29) - 1)
            out.append(([u] * (n - 1) + [0], [u] * (n - 1) + [0], c))
    return out


def mul_cases(F, op, rng):
    arity = OPS[op][1]
    out = [tuple(list(x) for x in t) for t in recorded().get((F.name, MUL_FORMS[op][0]), [])]
    out += class_lanes(F, op)
    sm = small(F)
    for t, a in enumerate(sm):
        out.append(tuple([a] + [sm[(t + 3 * j) % len(sm)] for j in range(1, arity)]))
        out.append(tuple([a] * arity))
    fill = []
    while len(out) + len(fill) < MIN_LANES or len(fill) < 64:
        cls = CLASSES[op][len(fill) % len(CLASSES[op])]
        ops = tuple([rng.randrange(_cls_max(b) + 1) for _ in range(F.NL - 1)] + [rng.randrange(1 << (b - 10))] for b in cls)
        fill.append(ops)
    return out + fill


# ------------------------------------------------------------------------------- zero tests, by wave
def compose(zeros, filtered, passing, rng):
    """64-lane groups: no candidate; interleaved; one zero in lane 0; one in lane 63 (the first 256 lanes);
    then every zero in all-zero groups, the passing nonzero lanes in groups of their own (candidates, no
    zero), and a partial last group of 37 mixed lanes. Returns (lanes, {group name: lane range})."""
    fi = iter(filtered)
    lanes, groups = [], {}

    def group(name, g):
        assert len(g) == 64 or name == "tail"
        groups[name] = range(len(lanes), len(lanes) + len(g))
        lanes.extend(g)

    group("none", [next(fi) for _ in range(64)])
    group("mixed", [zeros[(7 * t) % len(zeros)] if t % 2 == 0 else next(fi) for t in range(64)])
    group("lane0", [zeros[1 % len(zeros)]] + [next(fi) for _ in range(63)])
    group("lane63", [next(fi) for _ in range(63)] + [zeros[2 % len(zeros)]])
    z = list(zeros)
    while len(z) % 64:
        z.append(zeros[rng.randrange(len(zeros))])
    for t in range(0, len(z), 64):
        group(f"zeros{t // 64}", z[t:t + 64])
    q = list(passing)
    while len(q) % 64:
        q.append(passing[rng.randrange(len(passing))])
    for t in range(0, len(q), 64):
        group(f"pass{t // 64}", q[t:t + 64])
    group("tail", [(zeros, passing)[t % 2][rng.randrange(len((zeros, passing)[t % 2]))] if t % 3 else next(fi)
                   for t in range(37)])
    return lanes, groups


def zero_forms(F, k):
    """representations of k p inside fp_is_zero's precondition: normalized; a carry left in limb 0, the
    middle limb, limb NL - 2; KB_EQ - b for b a normalized and a loose multiple of p under KB_EQ"""
    n = F.limbs(k * F.p)
    out = [n] + [c for c in (carry_left(F, n, j) for j in (0, F.NL // 2, F.NL - 2)) if c]
    K = F.C["KB_EQ"]
    m = F.KB["KB_EQ"][0] - k
    if m >= 0:
        for b in (F.limbs(m * F.p), dominated(F, K, m * F.p), loosen(F, F.limbs(m * F.p), min(K[:-1]))):
            if b and all(x <= y for x, y in zip(b, K)) and F28.negk(F, "KB_EQ", b) not in out:
                out.append(F28.negk(F, "KB_EQ", b))
    return out


def is_zero_pools(F, rng):
    zeros = [z for k in range(F.kmax) for z in zero_forms(F, k)]
    lim = F.kmax * F.p
    filtered = []
    while len(filtered) < 400:
        x = rnd(F, rng, lim)
        if F28.filter_candidate(F, x) >= 256:
            filtered.append(loosen(F, x) if len(filtered) % 3 == 0 else x)
    passing = []
    top = 1 << (F.LB * (F.NL - 1))
    for k in range(F.kmax):
        for d in (1 << F.LB, -(1 << F.LB), top, -top, rng.randrange(1, F.p >> F.LB) << F.LB, 1, -1):
            v = k * F.p + d
            if 0 <= v < lim:
                passing.append(F.limbs(v))
                assert abs(d) == 1 or F28.filter_candidate(F, passing[-1]) == k
    return [(z,) for z in zeros], [(x,) for x in filtered], [(x,) for x in passing]


def eq_pools(F, rng):
    """a = b + j p in different redundant forms (equal), near misses b + j p + d that pass the filter, and
    unrelated pairs; b under KB_EQ, a + KB_EQ - b inside fp_is_zero's precondition"""
    K, (mult, limb, dom) = F.C["KB_EQ"], F.KB["KB_EQ"]
    jmax = F.kmax - mult
    bmax = int(dom * F.p) if F is BN254 else 63 * F.p

    def b_forms(v):
        forms = [F.limbs(v)] if F is BN254 else [F.limbs(v), loosen(F, F.limbs(v), limb), dominated(F, K, v)]
        return [b for b in forms if b and all(x <= y for x, y in zip(b, K))]

    def a_forms(v):
        n = F.limbs(v)
        return [n] + [c for c in (carry_left(F, n, j) for j in (0, F.NL // 2, F.NL - 2)) if c] + [loosen(F, n, 1 << 30)]

    equal, near, other = [], [], []
    top = 1 << (F.LB * (F.NL - 1))
    vals = [0, 1, F.p - 1, F.p, bmax - 1] + [rng.randrange(bmax) for _ in range(40)]
    for t, vb in enumerate(vals):
        for j in sorted({0, 1, jmax - 1, rng.randrange(jmax)}):
            bs, as_ = b_forms(vb), a_forms(vb + j * F.p)
            for u, b in enumerate(bs):
                equal.append((as_[(t + u) % len(as_)], b))
            for d in (1 << F.LB, -(1 << F.LB), top, -top, 1, -1):
                if vb + j * F.p + d >= 0 and (vb + j * F.p + d) // F.p < jmax:
                    near.append((F.limbs(vb + j * F.p + d), bs[t % len(bs)]))
    while len(other) < 400:
        a, b = rnd(F, rng, jmax * F.p), rnd(F, rng, bmax)
        if F28.filter_candidate(F, F28.subk(F, "KB_EQ", a, b)) >= 256:
            other.append((a, b))
    return equal, other, near


def f30_zero_pools(rng):
    K, p, n = L.ZK, L.P, L.N

    def forms(x):
        d = L.digits(x)
        out = [d]
        for j in (0, n // 2, n - 2):  # a doubled-size digit: digit j + 2^30, digit j+1 - 1, and the other way
            for s in (1, -1):
                r = list(d)
                r[j] += s << 30
                r[j + 1] -= s
                out.append(r)
                r = list(d)  # digit j -+ 2^31 where that fits int32: a magnitude of 2^31 - 2^29 or more
                r[j] += s << 31
                r[j + 1] -= 2 * s
                if -(1 << 31) < r[j] < (1 << 31):
                    out.append(r)
        assert all(L.val(r) == x for r in out)
        return out

    zeros = [z for k in range(-K, K + 1) for z in forms(k * p)]
    filtered, passing = [], []
    while len(filtered) < 400:
        z = L.digits(rng.randrange(-K * p, K * p + 1))
        if len(filtered) % 4 == 0:  # a digit at +-(2^31 - 1), which no multiple of p's digits need hold
            z[(len(filtered) // 4) % (n - 1)] = (-1) ** (len(filtered) // 8) * ((1 << 31) - 1)
        if not -K <= L.sext((z[0] & U32) * ((-L.PINV30) & U32), 30) <= K and abs(L.val(z)) <= K * p:
            filtered.append(z)
    for k in range(-K, K + 1):
        for d in (1 << 30, -(1 << 30), 1 << 360, -(1 << 360), rng.randrange(1, p >> 30) << 30, 1, -1):
            if abs(k * p + d) <= K * p:
                passing += forms(k * p + d)[:3]
    return [(_u(z),) for z in zeros], [(_u(z),) for z in filtered], [(_u(z),) for z in passing]


# ------------------------------------------------------------------------------- the other ops
def _kp_edges(F):
    ks = [1, 2, 4, 8, 16, 32, 64, 128, 255]
    vals = [0] + [k * F.p + d for k in ks if k < F.kmax for d in (-1, 0, 1)] + [F.kmax * F.p - 1]
    return [v for v in vals if 0 <= v < F.kmax * F.p]


def special(F, op, rng):
    """(edge operand tuples, a generator of one random filler tuple) for the ops that are neither multiply
    forms nor zero tests"""
    p, n, lim = F.p, F.NL, F.kmax * F.p
    N = F.limbs
    red = [0, 1, p - 1, p, p + 1, 2 * p - 1]
    if op == "fp_reduce_canon":
        return [(N(v),) for v in _kp_edges(F)], lambda: (rnd(F, rng, lim),)
    if op in ("fp_canon", "fp_norm"):
        e = [f for v in _kp_edges(F) for f in (N(v), loosen(F, N(v)), loosen(F, N(v), 1 << 30))]
        e += [c for v in _kp_edges(F)[1:] for c in (carry_left(F, N(v), j) for j in (0, n // 2, n - 2)) if c]
        return [(x,) for x in e], lambda: (loosen(F, rnd(F, rng, lim), rng.choice([CAP, 1 << 31, 1 << 29])),)
    if op == "fp_reduce_once":
        return [(N(v),) for v in red], lambda: (rnd(F, rng, 2 * p),)
    if op == "fp_cond_sub_2p":
        return [(N(v),) for v in red + [2 * p, 2 * p + 1, 3 * p, 4 * p - 1]], lambda: (rnd(F, rng, 4 * p),)
    if op == "fp_half":
        tmax = (1 << 32) - 2 - F.PL[-1]  # top + p's top + 1 < 2^32
        run = [(1 << F.LB) - F.PL[0]] + [F.MASK - x for x in F.PL[1:-1]]  # odd; the + p carry runs through every limb
        e = [N(v) for v in red + [2, 3 * p - 2]] + [run + [0], run + [tmax], [F.MASK] * (n - 1) + [tmax],
                                                     [F.MASK - 1] * (n - 1) + [tmax], [1] + [0] * (n - 2) + [tmax]]
        return [(x,) for x in e], lambda: ([rng.randrange(F.MASK + 1) for _ in range(n - 1)] + [rng.randrange(tmax + 1)],)
    if op in ("fp_add_red", "fp_sub_red"):
        e = [(N(a), N(a)) for a in red] + [(N(0), N(2 * p - 1)), (N(2 * p - 1), N(2 * p - 1)), (N(2 * p - 1), N(0)),
                                            (N(p), N(p - 1)), (N(p - 1), N(p)), (N(1), N(2))]
        return e, lambda: (rnd(F, rng, 2 * p), rnd(F, rng, 2 * p))
    if op in ("fp_lt_canon", "fp_neg_canon"):
        c = [0, 1, 2, p - 1, p - 2, p >> 1] + [rng.randrange(p) for _ in range(4)]
        if op == "fp_neg_canon":
            return [(N(v),) for v in c] + [(_unit(F, k),) for k in range(n)], lambda: (rnd(F, rng, p),)
        e = [(N(a), N(b)) for a in c[:6] for b in c[:6]]
        for v in c[5:]:  # operands that differ in one limb only, both ways
            for k in range(n):
                w = v ^ (1 << (F.LB * k + 3))
                if w < p:
                    e += [(N(v), N(w)), (N(w), N(v))]
        return e, lambda: (rnd(F, rng, p), rnd(F, rng, p))
    if op.startswith(("fp_subk_nr", "fp_negk_nr")):
        kname = op[op.index("<") + 1:-1]
        K, (_, limb, _) = F.C[kname], F.KB[kname]
        bs = [[0] * n, list(K), [limb] * (n - 1) + [K[-1]], [min(F.MASK, k) for k in K]]
        rb = lambda: [rng.randrange(k + 1) for k in K]
        if op.startswith("fp_negk_nr"):
            return [(b,) for b in bs], lambda: (rb(),)
        edge = [U32 - k for k in K]  # a + K at the edge of 32 bits
        as_ = [[0] * n, edge, [F.MASK] * n, N(p - 1)]
        return [(a, b) for a in as_ for b in bs], lambda: ([rng.randrange(x + 1) for x in edge], rb())
    if op == "fp_from_words":
        full = 1 << (32 * F.NW)
        vals = [0, 1, p - 1, p, full - 1, full >> 1] + [1 << (F.LB * k) for k in range(n)] + [(1 << (F.LB * k)) - 1 for k in range(1, n)]
        W = lambda v: [(v >> (32 * k)) & U32 for k in range(F.NW)]
        return [(W(v),) for v in vals], lambda: (W(rng.randrange(full)),)
    if op == "fp_to_words":
        full = 1 << (32 * F.NW)
        vals = [0, 1, p - 1, p, full - 1, full >> 1] + [1 << (F.LB * k) for k in range(n)] + [(1 << (32 * k)) - 1 for k in range(1, F.NW)]
        return [(N(v),) for v in vals], lambda: (rnd(F, rng, full),)
    if op in ("fp_to_mont", "fp_from_mont"):
        e = small(F) + [[F.MASK] * n, N(2 * p - 1)]
        return [(x,) for x in e], lambda: ([rng.randrange(F.MASK + 1) for _ in range(n)],)
    if op == "fp_add":
        half = (1 << 31) - 16  # two such limbs and a carry stay inside 32 bits
        e = small(F) + [[F.MASK] * n, [half] * (n - 1) + [F.MASK]]
        return [(a, b) for a in e for b in e[-3:]], lambda: (loosen(F, rnd(F, rng, lim >> 1), half), loosen(F, rnd(F, rng, lim >> 1), half))
    if op in ("f_mul(fp2)", "f_sqr(fp2)"):
        k = OPS[op][1]
        e = [N(v) for v in red] + [F.C["ONE"]]
        edges = [tuple(e[(t + 2 * j) % len(e)] for j in range(k)) for t in range(len(e))] + [tuple([x] * k) for x in e]
        return edges, lambda: tuple(rnd(F, rng, 2 * p) for _ in range(k))
    if op == "f30_from_fp":
        hi = (1 << 383) - 1
        e = [N(0), N(1), N(p), N(hi), loosen(F, N(hi)), loosen(F, N(hi), 1 << 30), loosen(F, N(p)), [CAP] * (n - 1) + [0],
             loosen(F, N(hi - (1 << 382)))]
        e += [N(sum((1 << 29) << (30 * k) for k in range(12))), N(sum(((1 << 29) - 1) << (30 * k) for k in range(12)))]
        return [(x,) for x in e], lambda: (loosen(F, rnd(F, rng, hi + 1), rng.choice([CAP, 1 << 28, 1 << 30])),)
    if op in ("fp_from_f30", "fp_mont_from_f30<1>", "fp_mont_from_f30<2>"):
        lo, hi = (-p + 1, p - 1) if op == "fp_from_f30" else (0, F28.P_1001 - 1)
        vals = [lo, hi, 0, 1, p - 1, hi - 1] + ([-1, p // 2, -(p // 2)] if lo < 0 else [p])
        e = [L.digits(v) for v in vals if lo <= v <= hi]
        for signs in ([1] * 12, [-1] * 12, [(-1) ** k for k in range(12)], [-(-1) ** k for k in range(12)]):
            low = sum(s * (1 << 29) << (30 * k) for k, s in enumerate(signs))  # every lower digit at +-2^29
            t0, t1 = -((low - lo) >> 360), (hi - low) >> 360  # the first and the last top digit inside the range
            e += [[s << 29 for s in signs] + [t] for t in (t0, t1, (t0 + t1) // 2)]
        assert all(lo <= L.val(z) <= hi for z in e)
        return [(_u(z),) for z in e], lambda: (_u(L.digits(rng.randrange(lo, hi + 1))),)
    if op in ("f30_from_mont<1>", "f30_from_mont<2>"):
        vals = [0, 1, 2, 3, p - 1, p, p + 1, F28.P_1001 - 1, F28.P_1001 - 2]
        return [(N(v),) for v in vals], lambda: (rnd(F, rng, F28.P_1001),)
    raise KeyError(op)


# ------------------------------------------------------------------------------- cases, computed once
_cases = {}


def cases(op, field):
    """(operand tuples, expected result words, wave groups or None), once per (op, field)"""
    key = (op, field)
    if key not in _cases:
        F = F28.FIELD[field]
        rng = random.Random(f"{op}/{field}")
        groups = None
        if op in MUL_FORMS:
            ops = mul_cases(F, op, rng)
        elif op == "fp_is_zero":
            ops, groups = compose(*is_zero_pools(F, rng), rng)
        elif op == "fp_eq":
            ops, groups = compose(*eq_pools(F, rng), rng)
        elif op == "f30_is_zero<16>":
            ops, groups = compose(*f30_zero_pools(rng), rng)
        else:
            ops, fill = special(F, op, rng)
            ops = list(ops)
            while len(ops) < MIN_LANES:
                ops.append(fill())
        if len(ops) % 64 == 0:
            ops.append(ops[0])
        model = OPS[op][5]
        _cases[key] = (ops, [list(model(F, *o)) for o in ops], groups)
    return _cases[key]


PAIRS = [(op, f) for op in OPS for f in OPS[op][2]]
IDS = [f"{op}-{f}" for op, f in PAIRS]


# ------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def fp_op(gpu):
    from kzgpot import _lib

    lib = ctypes.CDLL(_lib.TEST_LIB_PATH)
    fn = lib.kzgpot_test_fp_op
    fn.restype = ctypes.c_int
    ptr = ctypes.POINTER(ctypes.c_uint32)
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_long] + [ptr] * 7

    def run(op, field, ops):
        code, arity, _, inw, outw, _ = OPS[op]
        F = F28.FIELD[field]
        width = {"L": F.NL, "LL": 2 * F.NL, "W": F.NW, "D": L.N, "P": 1}
        iw, ow = width[inw], width[outw]
        assert all(len(a) == iw for o in ops for a in o) and all(len(o) == arity for o in ops)
        n = len(ops)
        bufs = []
        for j in range(6):
            if j < arity:
                flat = [x for o in ops for x in o[j]]
                bufs.append((ctypes.c_uint32 * len(flat))(*flat))
            else:
                bufs.append(None)
        out = (ctypes.c_uint32 * (ow * n))()
        rc = fn(code, BOTH.index(field), n, *bufs, out)
        assert rc == 0, rc
        return [list(out[ow * i:ow * i + ow]) for i in range(n)]

    return run


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", ["256", "all"])
@pytest.mark.parametrize("op,field", PAIRS, ids=IDS)
def test_limbs_exact(fp_op, op, field, lanes):
    ops, want, _ = cases(op, field)
    n = 256 if lanes == "256" else len(ops)
    assert n <= len(ops) and (lanes == "256" or n % 64)
    got = fp_op(op, field, ops[:n])
    bad = [i for i in range(n) if got[i] != want[i]]
    assert not bad, (f"{op} ({field}): lane {bad[0]} (of {len(bad)} wrong lanes in {n}) differs: operands "
                     f"{[[hex(x) for x in o] for o in ops[bad[0]]]}, got {[hex(x) for x in got[bad[0]]]}, "
                     f"want {[hex(x) for x in want[bad[0]]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("h", [1, 2])
def test_mont_f30_round_trip(fp_op, h):
    """fp_mont_from_f30<H> of the device's own f30_from_mont<H> digits is the same element, normalized and
    below 1.01 p; f30_from_fp then fp_from_f30 gives a canonical value back unchanged"""
    ops, _, _ = cases(f"f30_from_mont<{h}>", "bls12_381")
    z = fp_op(f"f30_from_mont<{h}>", "bls12_381", ops)
    back = fp_op(f"fp_mont_from_f30<{h}>", "bls12_381", [(d,) for d in z])
    for i, ((a,), r) in enumerate(zip(ops, back)):
        assert (BLS.val(r) - BLS.val(a)) % BLS.p == 0 and BLS.val(r) < BLS.p + BLS.p // 100, (h, i, a, r)
        assert all(x <= BLS.MASK for x in r[:-1])
    canon = [o for o in ops if BLS.val(o[0]) < BLS.p]
    z = fp_op("f30_from_fp", "bls12_381", canon)
    back = fp_op("fp_from_f30", "bls12_381", [(d,) for d in z])
    assert back == [o[0] for o in canon]


# ------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("op,field", PAIRS, ids=IDS)
def test_operands_inside_the_model(op, field):
    """every operand set passes the model's range checks (building the cases runs the model on each), and
    the results are the integers the functions stand for"""
    F = F28.FIELD[field]
    ops, want, groups = cases(op, field)
    assert len(ops) >= MIN_LANES and len(ops) % 64 and len(ops) < 4000
    assert all(0 <= x <= U32 for o in ops for a in o for x in a)
    v = [[F.val(a) for a in o] for o in ops]
    for i, (o, r) in enumerate(zip(ops, want)):
        if op in MUL_FORMS:
            assert (F.val(r) * F.R - MUL_FORMS[op][1](v[i])) % F.p == 0 and all(x <= F.MASK for x in r), i
        elif op in ("fp_is_zero",):
            assert r == [int(v[i][0] % F.p == 0)] and v[i][0] < F.kmax * F.p and max(o[0]) <= CAP, i
        elif op == "fp_eq":
            assert r == [int((v[i][0] - v[i][1]) % F.p == 0)], i
            d = F28.subk(F, "KB_EQ", *o)  # b under KB_EQ, the difference inside fp_is_zero's precondition
            assert all(b <= k for b, k in zip(o[1], F.C["KB_EQ"])) and F.val(d) < F.kmax * F.p and max(d) <= CAP, i
        elif op == "f30_is_zero<16>":
            assert r == [int(L.val([_s32(x) for x in o[0]]) % F.p == 0)], i
        elif op in ("fp_canon", "fp_reduce_canon"):
            assert r == F.limbs(v[i][0] % F.p), i
        elif op == "fp_norm":
            assert r == F.limbs(v[i][0]), i
        elif op == "fp_reduce_once":
            assert r == F.limbs(v[i][0] % F.p) and v[i][0] < 2 * F.p, i
        elif op == "fp_cond_sub_2p":
            assert r == F.limbs(v[i][0] % (2 * F.p)) and v[i][0] < 4 * F.p, i
        elif op == "fp_half":
            assert (2 * F.val(r) - v[i][0]) % F.p == 0 and all(x <= F.MASK for x in r[:-1]), i
        elif op == "fp_add_red":
            assert r == F.limbs((v[i][0] + v[i][1]) % (2 * F.p)) and max(v[i]) < 2 * F.p, i
        elif op == "fp_sub_red":
            d = v[i][0] - v[i][1]
            assert r == F.limbs(d + 2 * F.p if d < 0 else d) and max(v[i]) < 2 * F.p, i
        elif op == "fp_lt_canon":
            assert r == [int(v[i][0] < v[i][1])] and max(v[i]) < F.p, i
        elif op == "fp_neg_canon":
            assert r == F.limbs(-v[i][0] % F.p) and v[i][0] < F.p, i
        elif op.startswith("fp_subk_nr"):
            K = F.C[op[op.index("<") + 1:-1]]
            assert r == [a + k - b for a, k, b in zip(o[0], K, o[1])] and all(b <= k for b, k in zip(o[1], K)), i
        elif op.startswith("fp_negk_nr"):
            K = F.C[op[op.index("<") + 1:-1]]
            assert r == [k - b for k, b in zip(K, o[0])] and min(r) >= 0, i
        elif op == "fp_from_words":
            assert F.val(r) == sum(w << (32 * k) for k, w in enumerate(o[0])) and F28.to_words(F, r) == o[0], i
        elif op == "fp_to_words":
            assert sum(w << (32 * k) for k, w in enumerate(r)) == v[i][0] and F28.from_words(F, r) == o[0], i
        elif op == "fp_to_mont":
            assert (F.val(r) - v[i][0] * F.R) % F.p == 0, i
        elif op == "fp_from_mont":
            assert r == F.limbs(v[i][0] * pow(F.R, -1, F.p) % F.p), i
        elif op == "fp_add":
            assert r == F.limbs(v[i][0] + v[i][1]), i
        elif op == "f_mul(fp2)":
            a0, a1, b0, b1 = v[i]
            c0, c1 = F.val(r[:F.NL]), F.val(r[F.NL:])
            assert (c0 * F.R - (a0 * b0 - a1 * b1)) % F.p == 0 and (c1 * F.R - (a0 * b1 + a1 * b0)) % F.p == 0, i
            assert max(c0, c1) < 2 * F.p and all(x <= F.MASK for x in r), i
        elif op == "f_sqr(fp2)":
            a0, a1 = v[i]
            c0, c1 = F.val(r[:F.NL]), F.val(r[F.NL:])
            assert (c0 * F.R - (a0 * a0 - a1 * a1)) % F.p == 0 and (c1 * F.R - 2 * a0 * a1) % F.p == 0, i
            assert max(c0, c1) < 2 * F.p and all(x <= F.MASK for x in r), i
        elif op == "f30_from_fp":
            d = [_s32(x) for x in r]
            assert L.val(d) == v[i][0] < 1 << 383 and max(o[0]) <= CAP and all(-(1 << 29) <= x < 1 << 29 for x in d[:-1]), i
            if v[i][0] < F.p:  # round trip
                assert F28.fp_from_f30(d) == F.limbs(v[i][0]), i
        elif op == "fp_from_f30":
            z = L.val([_s32(x) for x in o[0]])
            assert r == F.limbs(z % F.p) and -F.p < z < F.p, i
            assert L.val(F28.f30_from_fp(r)) == z % F.p, i
        elif op.startswith("f30_from_mont"):
            h = int(op[-2])
            d = [_s32(x) for x in r]
            assert (L.val(d) << h) % F.p == v[i][0] % F.p and 0 <= L.val(d) < F28.P_1001, i
            assert (F.val(F28.fp_mont_from_f30(h, d)) - v[i][0]) % F.p == 0, i
        elif op.startswith("fp_mont_from_f30"):
            h = int(op[-2])
            z = L.val([_s32(x) for x in o[0]])
            assert (F.val(r) - (z << h)) % F.p == 0 and F.val(r) < F.p + F.p // 100 and 0 <= z < F28.P_1001, i
        else:
            raise AssertionError(f"no property stated for {op}")


def test_recorder_yields_every_site():
    """at least the 716 distinct BLS12-381 operand-bound tuples of the proofs' entry points, every one of
    them a lane with every limb at its bound; the recorder is off and the field restored afterwards.
    The floors are counts of the recorder as it was when it was added (909 tuples: mul 396, mul_sum2 372,
    sqr 85, mul_sum3 34, mul_add8sqr 13, mul_addsqr 9; a count of 397 fp_mul sites includes the deliberate
    overflow of test_bounds_model_catches_overflow, which is not driven), taken again on that tree, per
    entry point, with the two entry points left out that proved ladders no kernel runs and were removed
    with them: without test_g1_fast_ladders_w_closed (the radix-2^28 W-form G1 ladders) 308 / 363 / 47 /
    34 / 13 and no mul_addsqr (765); also without the second ladder of test_ladders_closed, whose base
    was a ladder state, 272 / 361 / 38 / 34 / 11 (716). No tuple that another entry point records left."""
    rec = recorded()
    assert M.RECORD is None and M.NL == 14 and M.P == BLS.p and M.C["P"] == BLS.PL
    count = {form: len(rec[("bls12_381", form)]) for form in ("mul", "mul_sum2", "sqr", "mul_sum3", "mul_add8sqr")}
    floor = {"mul": 272, "mul_sum2": 361, "sqr": 38, "mul_sum3": 34, "mul_add8sqr": 11}
    assert all(count[f] >= floor[f] for f in floor) and sum(count.values()) >= 716, count
    assert rec[("bn254", "mul")] and rec[("bn254", "sqr")]
    for op, (form, _) in MUL_FORMS.items():
        for field in OPS[op][2]:
            lanes = {tuple(tuple(a) for a in o) for o in cases(op, field)[0]}
            assert set(rec.get((field, form), [])) <= lanes, (op, field)
    M.mul(M.normalized(1), M.normalized(1))  # off: nothing is stored
    assert M.RECORD is None


@pytest.mark.parametrize("op", ["fp_mul", "fp_mul_sum2", "fp_mul_sum3"])
def test_a_column_reaches_2_63(op):
    """at least one lane drives an accumulator to 2^63 or beyond: a signed or 63-bit one would show"""
    peaks = []
    for o in cases(op, "bls12_381")[0]:
        st = {}
        OPS[op][5](BLS, *o, stats=st)
        peaks.append(st["peak"])
    assert max(peaks) >= 1 << 63 and max(peaks) < 1 << 64


@pytest.mark.parametrize("op", sorted(MUL_FORMS))
def test_cases_have_teeth(op):
    """the same scan with a 63-bit accumulator — and, for the squaring forms, without the doubling of the
    cross products — differs from the exact model on at least one lane"""
    ops, want, _ = cases(op, "bls12_381")
    model = OPS[op][5]
    assert any(model(BLS, *o, bits=63) != w for o, w in zip(ops, want))
    assert all(model(BLS, *o, bits=64) == w for o, w in zip(ops[:50], want))
    if op in ("fp_sqr", "fp_mul_addsqr<8>"):
        assert any(model(BLS, *o, doubling=False) != w for o, w in zip(ops, want))


def test_sqr_limit():
    """why fp_sqr's class is 30 bits with single limbs at 2^31 - 1: every limb there leaves uint64, and a
    limb of 2^31 cannot be doubled"""
    n = BLS.NL
    with pytest.raises(OverflowError):
        F28.sqr(BLS, [(1 << 31) - 1] * (n - 1) + [0])
    with pytest.raises(OverflowError):
        F28.sqr(BLS, [1 << 31] + [0] * (n - 1))
    with pytest.raises(OverflowError):  # the result would not fit NL limbs
        F28.mul(BLS, [0] * (n - 1) + [CAP], [0] * (n - 1) + [CAP])
    F28.sqr(BLS, [(1 << 30) - 1] * (n - 1) + [0])


@pytest.mark.parametrize("op,field", [("fp_is_zero", "bls12_381"), ("fp_is_zero", "bn254"), ("fp_eq", "bls12_381"),
                                      ("fp_eq", "bn254"), ("f30_is_zero<16>", "bls12_381")])
def test_zero_cases_are_composed_by_wave(op, field):
    F = F28.FIELD[field]
    ops, want, g = cases(op, field)
    z = [w[0] for w in want]

    def candidate(o):
        if op == "f30_is_zero<16>":
            return -L.ZK <= L.sext((o[0][0] & U32) * ((-L.PINV30) & U32), 30) <= L.ZK
        return F28.filter_candidate(F, o[0] if op == "fp_is_zero" else F28.subk(F, "KB_EQ", *o)) < 256

    c = [candidate(o) for o in ops]
    assert all(not z[i] or c[i] for i in range(len(ops)))  # no zero is filtered out
    assert [g[k] for k in ("none", "mixed", "lane0", "lane63")] == [range(64 * t, 64 * t + 64) for t in range(4)]
    assert not any(c[i] for i in g["none"])                                       # the wave takes the early exit
    assert [z[i] for i in g["mixed"]] == [1, 0] * 32
    assert [z[i] for i in g["lane0"]] == [1] + [0] * 63 and [c[i] for i in g["lane0"]] == [True] + [False] * 63
    assert [z[i] for i in g["lane63"]] == [0] * 63 + [1] and [c[i] for i in g["lane63"]] == [False] * 63 + [True]
    zero_groups = [k for k in g if k.startswith("zeros")]
    pass_groups = [k for k in g if k.startswith("pass")]
    assert zero_groups and all(z[i] for k in zero_groups for i in g[k])
    assert pass_groups and not any(z[i] for k in pass_groups for i in g[k])
    assert sum(c[i] for k in pass_groups for i in g[k]) >= 32                     # nonzero values that pass the filter
    assert len(g["tail"]) == 37 and g["tail"][-1] == len(ops) - 1
    if op == "fp_is_zero":  # every k the precondition allows, in every form that exists for it
        ks = {F.val(ops[i][0]) // F.p for k in zero_groups for i in g[k]}
        assert ks == set(range(F.kmax)) and F.kmax == (256 if field == "bls12_381" else 169)
        assert sum(len(g[k]) for k in zero_groups) >= 4 * F.kmax
    if op == "f30_is_zero<16>":
        ks = {L.val([_s32(x) for x in ops[i][0]]) // F.p for k in zero_groups for i in g[k]}
        assert ks == set(range(-L.ZK, L.ZK + 1))
        big = (1 << 31) - (1 << 29)
        assert any(_s32(x) >= big for k in zero_groups for i in g[k] for x in ops[i][0])
        assert any(_s32(x) <= -big for k in zero_groups for i in g[k] for x in ops[i][0])
        assert {(1 << 31) - 1, -(1 << 31) + 1} <= {_s32(x) for o in ops for x in o[0]}
