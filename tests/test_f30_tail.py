"""The tail forms of the radix-2^30 scans and the G1 subgroup ladders that run them (csrc/fp381.hpp
f30_mul<K0, K1> / f30_sqr<K0, K1>; csrc/curve.hpp jac<f30>), CPU only, on the exact model of
tests/f30_tail_model.py:

1. the tail scan: without tails the plain scan digit for digit; with tails the SAME INTEGER as the form
   it replaced (plain scan, digit-wise difference, f30_norm), at random and extreme digits, with
   balanced output digits and the top digit inside its bound;
2. every column of every call site inside int64 for every input in the stated bound set, and the set
   closed under a ladder step, entered by the tripling of either ladder's base — the statement
   tests/test_f30_ladder.py makes for the forms without tails;
3. the formulas' algebra against plain affine arithmetic, the exceptional branches included, the
   whole endomorphism test's accept / reject, and each step against the former model's step.
"""
import random

import pytest

import f30_ladder_model as M
import f30_tail_model as T
import test_f30_ladder as L
from f30_ladder_model import B, P, R30, V, val

B_D, STATE = L.B_D, L.STATE
TOP = 1 << 23


def _rand(rng, d=B_D, top=TOP):
    return [rng.randrange(-d, d + 1) for _ in range(12)] + [rng.randrange(-top, top + 1)]


def _extreme(t, d=B_D, top=TOP):
    return [(d if (t >> (k % 3)) & 1 else -d) for k in range(12)] + [top if t & 1 else -top]


def _v(d, dmax=B_D, top=TOP):
    return V(d, B(dmax, top, abs(val(d)) + 1))


# ------------------------------------------------------------------------------- 1. the tail scan
def test_scan_without_tails_is_the_plain_scan():
    rng = random.Random(4001)
    for t in range(60):
        mk = (lambda: _extreme(rng.randrange(8))) if t < 16 else (lambda: _rand(rng))
        a, b, c = mk(), mk(), mk()
        assert T.scan([(a, b)], []) == M._scan([(a, b)], [])
        assert T.scan([], [c]) == M._scan([], [c])
        assert T.scan([(a, b)], [c]) == M._scan([(a, b)], [c])


# the forms the ladders use: (tail factors, the former steps on the plain product s and the tails)
FORMS = {
    "dbl_x3": ((-2,), lambda s, t: M.norm(M.sub(s, M.dbl(t[0])))),
    "madd_h": ((-1,), lambda s, t: M.norm(M.sub(s, t[0]))),
    "madd_x3": ((-1, -2), lambda s, t: M.norm(M.sub(M.norm(M.sub(M.sub(s, t[0]), t[1])), t[1]))),
    "tpl_u": ((-1, -1), lambda s, t: M.norm(M.sub(M.norm(M.sub(s, t[0])), t[1]))),
}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("op", ["mul", "sqr"])
def test_tail_form_is_the_former_integer(form, op):
    """value(tail form) == value(plain scan, difference, f30_norm) as integers, not only mod p"""
    ks, former = FORMS[form]
    rng = random.Random(4002 + len(form))
    for t in range(200):
        mk = (lambda: _extreme(rng.randrange(8))) if t < 48 else (lambda: _rand(rng))
        a, b = _v(mk()), _v(mk())
        # the tails are products (D, J, V, MM, EE) or, for H and r, a ladder coordinate; the former
        # doubling's f30_norm takes F - 2D only for a product D, digits in [-2^29, 2^29)
        tails = [V([max(-(1 << 29), min((1 << 29) - 1, x)) for x in mk()[:-1]] + [rng.randrange(-TOP, TOP + 1)],
                   B(1 << 29, TOP, 1 << 384, (1 << 29) - 1)) for _ in ks]
        if op == "mul":
            got, plain = T.mul_tail(a, b, *zip(ks, tails)), M.mul(a, b)
        else:
            got, plain = T.sqr_tail(a, *zip(ks, tails)), M.sqr(a)
        assert val(got.d) == val(plain.d) + sum(k * val(x.d) for k, x in zip(ks, tails))
        assert val(got.d) == val(former(plain, tails).d)
        assert all(-(1 << 29) <= x < (1 << 29) for x in got.d[:-1])
        assert abs(got.d[-1]) <= got.b.top


def test_tail_carries_cross_every_digit_boundary():
    """a tail that lifts or lowers each column's sum past +-2^29 changes that column's carry by
    exactly one and leaves the integer right: digits +-2^29 in one position at a time, 64 t everywhere"""
    rng = random.Random(4003)
    a, b = _v(_rand(rng)), _v(_rand(rng))
    plain = M.mul(a, b)
    for k in range(13):
        for sgn in (1, -1):
            t = [0] * 13
            t[k] = sgn * (1 << 29) if k < 12 else sgn * TOP
            tv = V(t, B(1 << 29, TOP, abs(val(t)) + 1))
            for kk in (-2, -1, 1, T.K_MIN, T.K_MAX):
                got = T.mul_tail(a, b, (kk, tv))
                assert val(got.d) == val(plain.d) + kk * val(t)
                assert all(-(1 << 29) <= x < (1 << 29) for x in got.d[:-1])


def test_tail_bounds_are_checked():
    st = M.bound_only(STATE)
    T.sqr_tail(st, (-2, st))
    T.sqr_tail(st, (-1, st), (-2, st))
    T.mul_tail(st, M.dbl(st), (-1, st))  # one doubled operand, as f30_mul takes
    with pytest.raises(OverflowError):
        T.mul_tail(M.dbl(st), M.dbl(st), (-1, st))
    with pytest.raises(AssertionError):
        T.sqr_tail(st, (65, st))
    with pytest.raises(AssertionError):
        T.sqr_tail(st, (-1, st), (-1, st), (-1, st))
    # the tail is part of the column: a plain product that fits, pushed out by its tail alone (a
    # hypothetical 57-bit tail digit; the widest plain column is a lower one, which takes no tail)
    T.check_columns([(STATE, STATE)], [], "plain")
    with pytest.raises(OverflowError):
        T.check_columns([(STATE, STATE)], [(64, B(1 << 57, TOP, P))], "tail")
    # the top digit leaves int32 with a large enough tail value
    with pytest.raises(AssertionError):
        T.sqr_tail(st, (64, M.bound_only(B(1 << 29, 1 << 26, (1 << 26) << 360))))


# ------------------------------------------------------------------------------- 2. closed bound set
def _inside(vs):
    for v in vs:
        assert v.b.within(STATE), (v.b, STATE)


def test_bound_set_closed_under_a_ladder_step():
    """bounds-only runs: every product's worst-case column (tails included) inside int64, every
    f30_norm input inside int32, every zero test inside F30_ZK p, for EVERY state in the set"""
    assert M.top_from_value(STATE.v, STATE.d) < STATE.top
    s = [M.bound_only(STATE)] * 3
    base = M.bound_only(STATE)
    _inside(T.jac_tpl_affine_w(base, base))
    d = T.jac_dbl_w(*s)
    _inside(d)
    _inside(T.jac_madd_w(*d, base, base, decide=False))
    _inside(T.jac_dbl_w(*d))
    z = M.mul(s[2], s[2])
    xb = M.mul(M.bound_only(M.of_int(P - 1).b), M.of_int(val(M.HDR["BETA30"])))
    M.jac_eq_affine(s[0], s[1], z, xb, M.neg(base))


def test_call_sites_worst_columns():
    """the tail adds at most 3 * 2^29 to a column of ~2^62.7: recorded, and far inside int64"""
    st = M.bound_only(STATE)
    for r in (T.sqr_tail(st, (-2, st)), T.mul_tail(st, st, (-1, st)), T.sqr_tail(st, (-1, st), (-2, st)),
              T.sqr_tail(st, (-1, st), (-1, st))):
        assert r.worst < (1 << 63) - (1 << 60)
    plain = T.check_columns([(STATE, STATE)], [], "plain")
    assert T.sqr_tail(st, (-1, st), (-2, st)).worst - plain <= 3 * STATE.d + 3


# ------------------------------------------------------------------------------- 3. algebra
def test_steps_agree_with_the_former_model():
    """from the same state: X3 / H / r are the former integers; what is computed FROM them (other digits
    of the same integer, so another m) agrees mod p"""
    rng = random.Random(4004)
    for _ in range(4):
        pt = L.on_curve_point(rng)
        x, w = L.base30(pt)
        for new, old in ((T.jac_tpl_affine_w(x, w), M.jac_tpl_affine_w(x, w)),):
            assert [val(a.d) % P for a in new] == [val(a.d) % P for a in old]
        st = M.jac_tpl_affine_w(x, w)
        dn, do = T.jac_dbl_w(*st), M.jac_dbl_w(*st)
        assert val(dn[0].d) == val(do[0].d) and val(dn[2].d) == val(do[2].d)
        assert (val(dn[1].d) - val(do[1].d)) % P == 0
        an, ao = T.jac_madd_w(*do, x, w), M.jac_madd_w(*do, x, w)
        assert val(an[0].d) == val(ao[0].d) and val(an[2].d) == val(ao[2].d)
        assert (val(an[1].d) - val(ao[1].d)) % P == 0


def test_doubling_tripling_and_mixed_addition():
    rng = random.Random(4005)
    for _ in range(6):
        pt = L.on_curve_point(rng)
        x, w = L.base30(pt)
        t = T.jac_tpl_affine_w(x, w)
        assert L.jac_to_affine(*t) == L.aff_mul(3, pt)
        d = T.jac_dbl_w(*t)
        assert L.jac_to_affine(*d) == L.aff_mul(6, pt)
        assert L.jac_to_affine(*T.jac_madd_w(*d, x, w)) == L.aff_mul(7, pt)
        p6 = L.aff_mul(6, pt)
        assert L.jac_to_affine(*T.jac_madd_w(*d, *L.base30(p6))) == L.aff_mul(12, pt)   # equal-point branch
        m6 = (p6[0], P - p6[1])
        assert L.jac_to_affine(*T.jac_madd_w(*d, *L.base30(m6))) is None                # H = 0, r != 0
        inf = (d[0], d[1], M.of_int(0))
        assert L.jac_to_affine(*T.jac_madd_w(*inf, x, w)) == pt                         # z1zero branch


def test_ladder_abs_u_and_trace_within_closed_set():
    rng = random.Random(4006)
    for _ in range(3):
        pt = L.on_curve_point(rng)
        trace = []
        q = T.mul_abs_u_affine(*L.base30(pt), trace=trace)
        assert L.jac_to_affine(*q) == L.aff_mul(M.ABS_U, pt)
        for st in trace:
            for v in st:
                V(v.d, STATE)


def test_subgroup_test_accepts_and_rejects():
    rng = random.Random(4007)
    g = L.aff_mul(rng.randrange(1, L.R), L.G1)
    q = L.on_curve_point(rng)
    t3, t11 = L._torsion(rng, 3), L._torsion(rng, 11)
    cases = [(g, True), ((g[0], P - g[1]), True), (L.G1, True), (q, False), (L.aff_mul(L.R, q), False),
             (t3, False), (t11, False), ((0, 2), False), ((0, P - 2), False), (L.aff_add(g, t11), False)]
    for pt, want in cases:
        assert T.in_subgroup_fast_g1(*L.base30(pt)) is want, pt
        assert M.in_subgroup_fast_g1(*L.base30(pt)) is want
    for ell, t in ((3, t3), (11, t11)):  # mid-ladder infinity and the equal-point branch
        assert L.jac_to_affine(*T.mul_abs_u_affine(*L.base30(t))) == L.aff_mul(M.ABS_U % ell, t)
