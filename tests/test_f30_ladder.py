"""The G1 subgroup ladders on the radix-2^30 core (csrc/curve.hpp jac<f30>, csrc/fp381.hpp f30_*),
CPU only, on the exact model of tests/f30_ladder_model.py:

1. the new primitives, exact against Python integers, at random and extreme digits;
2. a bound set closed under one ladder step (doubling; doubling + mixed addition), which the
   tripling of either ladder's base enters — every product's worst-case columns inside int64 and
   every zero test inside its stated range for EVERY state in the set, not only the sampled ones;
3. the formulas' algebra against plain affine arithmetic mod p, the exceptional branches included,
   and the whole endomorphism test's accept / reject;
4. the zero test, exact over its whole stated range.
"""
import random

import pytest

import f30_ladder_model as M
from f30_ladder_model import B, P, R30, V, val

B_D = (1 << 29) + 4        # fp381.hpp: "balanced" = lower digits within 2^29 + 4
G1 = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
      0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
H1 = 0x396C8C005555E1568C00AAAB0000AAAB


# ------------------------------------------------------------------------------- plain curve math
def aff_add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % P == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, P) % P
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def aff_mul(k, p):
    acc = None
    while k:
        if k & 1:
            acc = aff_add(acc, p)
        p = aff_add(p, p)
        k >>= 1
    return acc


def on_curve_point(rng):
    while True:
        x = rng.randrange(P)
        y2 = (x * x * x + 4) % P
        y = pow(y2, (P + 1) // 4, P)
        if y * y % P == y2:
            return x, y if rng.randrange(2) else P - y


def to_r30(x):
    return M.of_int(x * R30 % P)


def base30(pt):
    """g1_park_base's output up to the representative: (x, w = 2y) in R30 form, balanced digits,
    values in [0, p). The device's values reach 1.001 p (test_park_and_unpark_conversions): the
    same residues, inside the same bound set."""
    return to_r30(pt[0]), to_r30(2 * pt[1] % P)


def from_r30(v):
    return val(v.d) * pow(R30, -1, P) % P


def jac_to_affine(X, W, Z):
    """(X : W/2 : Z) -> affine, None at infinity"""
    z = from_r30(Z)
    if z == 0:
        return None
    zi = pow(z, -1, P)
    return from_r30(X) * zi * zi % P, from_r30(W) * pow(2, -1, P) * zi ** 3 % P


# ------------------------------------------------------------------------------- 1. primitives
def _rand_balanced(rng, d=B_D, top=1 << 23):
    return [rng.randrange(-d, d + 1) for _ in range(12)] + [rng.randrange(-top, top + 1)]


def _extreme(t, d=B_D, top=1 << 23):
    return [(d if (t >> (k % 3)) & 1 else -d) for k in range(12)] + [top if t & 1 else -top]


def _v(d, dmax=B_D, top=1 << 23):
    return V(d, B(dmax, top, abs(val(d)) + 1))


def test_products_exact_random_and_extreme():
    rng = random.Random(3001)
    for t in range(300):
        mk = (lambda: _extreme(rng.randrange(8))) if t < 40 else (lambda: _rand_balanced(rng))
        a, b, c, d = (_v(mk()) for _ in range(4))
        for r, want in ((M.mul_sum2(a, b, c, d), val(a.d) * val(b.d) + val(c.d) * val(d.d)),
                        (M.mul_addsqr(a, b, c), val(a.d) * val(b.d) + val(c.d) ** 2),
                        (M.mul(a, b), val(a.d) * val(b.d)), (M.sqr(a), val(a.d) ** 2)):
            assert (val(r.d) * R30 - want) % P == 0
            assert all(-(1 << 29) <= x < (1 << 29) for x in r.d[:-1])


def test_product_with_one_doubled_operand():
    """f30_mul takes one digit-wise doubled balanced operand (the mixed addition's 2 Z1); the
    two-product forms do not: their columns leave int64 with it, and the model says so."""
    a = M.bound_only(B(B_D, 1 << 24, 8 * P))
    M.mul(M.dbl(a), a)
    with pytest.raises(OverflowError):
        M.mul_sum2(M.dbl(a), a, a, a)
    with pytest.raises(OverflowError):
        M.mul_addsqr(M.dbl(a), a, a)
    with pytest.raises(OverflowError):
        M.mul(M.dbl(a), M.dbl(a))


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_norm_exact(s):
    rng = random.Random(3002 + s)
    lim = (1 << 31) - (1 << (29 - s)) - 1
    for t in range(400):
        if t < 8:
            d = [lim if (t >> (k % 3)) & 1 else -lim - 1 for k in range(12)] + [(1 << 24) * (1 if t & 1 else -1)]
        else:
            d = [rng.randrange(-lim, lim + 1) for _ in range(12)] + [rng.randrange(-(1 << 24), 1 << 24)]
        r = M.norm(V(d, B(lim + 1, 1 << 24, abs(val(d)) + 1, lim)), s)
        assert val(r.d) == val(d) << s
        assert all(abs(x) <= (1 << 29) + (2 << s) for x in r.d[:-1])
    with pytest.raises(AssertionError):
        M.norm(M.bound_only(B(lim + 1, 1, P)), s)


# ------------------------------------------------------------------------------- 2. closed bound set
# The stated set: every coordinate of a ladder state, and either ladder's base (P's (x, w) in [0, p)
# from g1_park_base, or Q1's (X, W), itself a ladder state), is balanced with |top digit| <= 2^23 and
# |value| <= 4.5 p. (2^23 is what the exponentiation's TOP_IN happens to be; here it follows from
# the value bound: (4.5 p + lower digits) / 2^360 < 2^23.)
STATE = B(B_D, 1 << 23, 9 * P // 2)


def _inside(vs):
    for v in vs:
        assert v.b.within(STATE), (v.b, STATE)


def test_bound_set_closed_under_a_ladder_step():
    assert M.top_from_value(STATE.v, STATE.d) < STATE.top
    assert M.of_int(P - 1).b.within(STATE) and M.one().b.within(STATE)
    s = [M.bound_only(STATE)] * 3
    base = M.bound_only(STATE)
    _inside(M.jac_tpl_affine_w(base, base))              # the ladder's first step
    d = M.jac_dbl_w(*s)
    _inside(d)                                           # a doubling
    _inside(M.jac_madd_w(*d, base, base, decide=False))  # + a mixed addition: general branch,
    _inside(M.jac_dbl_w(*d))                             #   equal-point branch (and the infinity
    #                                                        branch loads (base, 1): inside, above)
    # the closing multiply and the comparison of in_subgroup_fast_g1, from any state in the set
    z = M.mul(s[2], s[2])
    xb = M.mul(M.bound_only(M.of_int(P - 1).b), M.of_int(val(M.HDR["BETA30"])))
    M.jac_eq_affine(s[0], s[1], z, xb, M.neg(base))


def test_constants():
    assert val(M.HDR["ONE30"]) == R30 % P
    beta = val(M.HDR["BETA30"]) * pow(R30, -1, P) % P
    assert beta != 1 and pow(beta, 3, P) == 1
    for name in ("ONE30", "BETA30"):
        assert all(-(1 << 29) <= d < (1 << 29) for d in M.HDR[name][:-1])


# ------------------------------------------------------------------------------- 3. algebra
def test_doubling_tripling_and_mixed_addition():
    rng = random.Random(3003)
    for _ in range(6):
        pt = on_curve_point(rng)
        x, w = base30(pt)
        t = M.jac_tpl_affine_w(x, w)
        assert jac_to_affine(*t) == aff_mul(3, pt)
        d = M.jac_dbl_w(*t)
        assert jac_to_affine(*d) == aff_mul(6, pt)
        assert jac_to_affine(*M.jac_madd_w(*d, x, w)) == aff_mul(7, pt)
        # equal-point branch: 6P + 6P through the mixed addition
        p6 = aff_mul(6, pt)
        assert jac_to_affine(*M.jac_madd_w(*d, *base30(p6))) == aff_mul(12, pt)
        # -6P: the sum is infinity (general branch, H = 0, r != 0 -> Z3 = 0)
        m6 = (p6[0], P - p6[1])
        assert jac_to_affine(*M.jac_madd_w(*d, *base30(m6))) is None
        # infinity + base: the z1zero branch
        inf = (d[0], d[1], M.of_int(0))
        assert jac_to_affine(*M.jac_madd_w(*inf, x, w)) == pt


def test_ladder_abs_u_and_trace_within_closed_set():
    rng = random.Random(3004)
    for _ in range(3):
        pt = on_curve_point(rng)
        trace = []
        q = M.mul_abs_u_affine(*base30(pt), trace=trace)
        assert jac_to_affine(*q) == aff_mul(M.ABS_U, pt)
        for st in trace:
            for v in st:
                V(v.d, STATE)  # asserts digits, top digit and value inside the stated set


def _torsion(rng, ell):
    """a point of order ell = 3 or 11: the whole ell-part of h1 = 3 * 11^2 * .. is cleared but one
    factor, and E(Fp)[11] = Z11 x Z11 (11 | u - 1), so [r h1 / 11^2] Q already has order 1 or 11"""
    e = 0
    while H1 % ell ** (e + 1) == 0:
        e += 1
    for _ in range(64):
        t = aff_mul(R * H1 // ell ** e, on_curve_point(rng))
        if t is not None:
            assert aff_mul(ell, t) is None
            return t
    raise AssertionError("no torsion point found")


def test_subgroup_test_accepts_and_rejects():
    rng = random.Random(3005)
    g = aff_mul(rng.randrange(1, R), G1)
    cases = [(g, True), ((g[0], P - g[1]), True), (G1, True)]
    q = on_curve_point(rng)
    cases.append((q, False))                                   # random on-curve point: outside G1
    cases.append((aff_mul(R, q), False))                       # pure cofactor torsion
    t3, t11 = _torsion(rng, 3), _torsion(rng, 11)
    cases += [(t3, False), (t11, False), ((0, 2), False), ((0, P - 2), False)]
    cases.append((aff_add(g, t11), False))                     # G + T
    for pt, want in cases:
        assert M.in_subgroup_fast_g1(*base30(pt)) is want, pt
        assert (aff_mul(R, pt) is None) is want


def test_mid_ladder_infinity():
    """A point of order 3 reaches infinity at the tripling; one of order 11 (|u| = 3 * 2^62 + ... is
    not a multiple) does not: both ladders still end where plain arithmetic ends."""
    rng = random.Random(3006)
    for ell in (3, 11):
        t = _torsion(rng, ell)
        assert aff_mul(ell, t) is None
        assert jac_to_affine(*M.mul_abs_u_affine(*base30(t))) == aff_mul(M.ABS_U % ell, t)


# ------------------------------------------------------------------------------- 4. zero test
def test_is_zero_exact_over_its_range():
    """|value| <= K p, any int32 digits: true exactly for the multiples of p. All 2K + 1 multiples,
    their neighbours, values that share a multiple's low digit (so the filter passes and the exact
    comparison decides), lazy digit forms of each, and random values."""
    rng = random.Random(3007)
    k_max = M.ZK

    def lazy(x):
        d = M.digits(x)
        for k in range(11, -1, -1):  # push multiples of 2^30 down: same value, digits up to ~2^31
            take = rng.randrange(-1, 2)
            d[k + 1] -= take
            d[k] += take << 30
        return V(d, B((1 << 31) - 1, (1 << 31) - 1, k_max * P))

    for k in range(-k_max, k_max + 1):
        for form in (lambda x: V(M.digits(x), B(1 << 29, (1 << 31) - 1, k_max * P)), lazy):
            assert M.is_zero(form(k * P)) is True
            for delta in (1, -1, 1 << 30, -(1 << 30), 1 << 360, (rng.randrange(1, 1 << 340) << 30)):
                x = k * P + delta
                if abs(x) <= k_max * P:
                    assert M.is_zero(form(x)) is False
    for _ in range(2000):
        x = rng.randrange(-k_max * P, k_max * P + 1)
        assert M.is_zero(V(M.digits(x), B(1 << 29, (1 << 31) - 1, k_max * P))) is (x % P == 0)
    # uniqueness of the candidate: two multiples of p within the range never share a low digit
    inv = pow(P, -1, 1 << 30)
    assert len({(k * P) % (1 << 30) for k in range(-k_max, k_max + 1)}) == 2 * k_max + 1
    assert (-M.PINV30) % (1 << 30) == inv
    with pytest.raises(AssertionError):
        M.is_zero(M.bound_only(B(1 << 29, 1 << 23, (k_max + 1) * P)))


# ------------------------------------------------------------------------------- 5. the parked point
def test_park_and_unpark_conversions():
    """g1_park_base (f30_from_mont<2> for x, <1> for y -> w = 2y) and the reference-ladder path's way
    back (fp_mont_from_f30), limb by limb. The device's inputs are Montgomery products (words_to_mont:
    value < 1.0004 p) or canonical, so the parked values lie in [0, 1.001 p), not only in [0, p) as
    base30() above has them: still balanced, and far inside the 4.5 p set."""
    rng = random.Random(3008)
    r28 = 1 << 392
    xs = [0, 1, P - 1, P, P + P // 1000 - 1, P + 1] + [rng.randrange(P + P // 1000) for _ in range(300)]
    for a in xs:
        for h in (1, 2):
            z = M.from_mont(h, M.limbs28(a))
            assert z.b.within(STATE)
            # R = 2^392 representative a of e  ->  R30 representative of 2^(2-h) e
            e = a * pow(r28, -1, P) % P
            assert val(z.d) % P == (e << (2 - h)) * R30 % P
            back = M.mont_from_f30(h, z)
            assert M.val28(back) % P == a % P
