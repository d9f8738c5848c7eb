"""Exact interval model of the radix-2^28 field arithmetic in csrc/fp381.hpp and the formulas in
csrc/curve.hpp / codec_kernels.hip / g1_kernels.hip — used by tests/test_field_bounds.py to PROVE (for all inputs)
that no 64-bit column accumulator, 32-bit limb or borrowed-constant subtraction can overflow.

Each value is modelled by per-limb upper bounds (exact ints) and a value upper bound (in units of
p, a float nudged upward at every step). The functions mirror the device code one to one, each formula
once: the Fp ladder of in_subgroup_ref<fp> / the group FFT / the MSM (jac_dbl, jac_madd, jac_eq_affine)
and the two Fp2 ladders (jac_dbl_fp2 / jac_madd_fp2, whose w is the template <bool W> of curve.hpp's
jac_dbl(jac<fp2>&) / jac_madd(jac<fp2>&, ..); jac_tpl_affine_fp2_w, jac_eq_affine_fp2). The G1 fast
ladders run on radix 2^30 and are proven in tests/f30_ladder_model.py.
"""
from __future__ import annotations

import os
import re
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kzg-setup-powersoftau_amd", "csrc")
CONSTS = os.path.join(CSRC, "bls12_381_consts.hpp")

FIELDS = {  # p, limbs, limb bits, constants header
    "bls12_381": (0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
                  14, 28, "bls12_381_consts.hpp"),
    "bn254": (0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47, 9, 29, "bn254_consts.hpp"),
}
UP = 1.0 + 1e-9  # upward nudge for float value bounds


def load_consts(path=CONSTS):
    """The integer constants of a constants header, by name: every one-dimensional array as a list, every
    scalar as an int (the one parser of the header: f30_ladder_model.py and test_fp30.py read through it)."""
    text = open(path).read()
    num = lambda v: int(v.strip().rstrip("uUlL"), 0)
    out = {n: num(v) for n, v in re.findall(r"constexpr u?int\w* (\w+) = (-?\w+);", text)}
    for name, body in re.findall(r"constexpr u?int\w* (\w+)\[\w+\] = \{([^{}]*)\}", text):
        out[name] = [num(v) for v in body.split(",")]
    return out


def use_field(name):
    """Point the model at a field (the device code is generic over the traits struct)."""
    global P, NL, LB, LM, R, P_L, P_OVER_R, P_TOP, C, _FIELD
    _FIELD = name
    P, NL, LB, hdr = FIELDS[name]
    LM = (1 << LB) - 1
    R = 1 << (LB * NL)
    P_L = [(P >> (LB * i)) & LM for i in range(NL)]
    P_OVER_R = P / R * UP
    P_TOP = P / (1 << (LB * (NL - 1))) * UP  # p / 2^364
    C = load_consts(os.path.join(CSRC, hdr))


use_field("bls12_381")


class BoundError(AssertionError):
    pass


# Recorder (off by default; tests/test_gpu_fp28_core.py switches it on): each multiply form stores the
# limb bounds of its operands, so that a value-level test can drive the device function with every limb
# AT the bound the proof claims. RECORD = None, or a dict (field, form, name) -> set of operand-bound
# tuples (one tuple of NL limb bounds per operand).
RECORD = None


def _record(form, name, *operands):
    if RECORD is not None:
        RECORD.setdefault((_FIELD, form, name), set()).add(tuple(tuple(v.limbs) for v in operands))


class V:
    """Upper bounds: limbs[i] >= every possible limb i; val >= value / p."""

    def __init__(self, limbs, val, name=""):
        self.limbs = list(limbs)
        self.val = float(val)
        self.name = name
        for i, l in enumerate(self.limbs):
            if l >= 1 << 32:
                raise BoundError(f"{name}: limb {i} may overflow 32 bits ({l:#x})")
        if self.val * P >= R * (1 - 1e-6):
            raise BoundError(f"{name}: value {float(self.val):.1f} p does not fit 392 bits")

    def __repr__(self):
        return f"V({self.name}: bits {max(l.bit_length() for l in self.limbs)}, v {float(self.val):.3f})"


def normalized(val, name=""):
    """A normalized value: limbs 0..12 < 2^28, top limb bounded by the value."""
    top = int(float(val) * P_TOP) + 1
    return V([LM] * (NL - 1) + [min(LM, top)], val, name)


def const(limbs, name=""):
    val = sum(l << (LB * i) for i, l in enumerate(limbs)) / P * UP
    return V(limbs, val, name)


def mont_output(val):
    return normalized(val)


def mul(a: V, b: V, name="mul"):
    """fp_mul: FIPS with one 64-bit accumulator per column (+ the m*p chain merged in)."""
    _record("mul", name, a, b)
    carry = 0
    for i in range(2 * NL):
        j0 = 0 if i < NL else i - (NL - 1)
        j1 = i if i < NL else NL - 1
        s = sum(a.limbs[j] * b.limbs[i - j] for j in range(j0, j1 + 1))
        s += sum(LM * P_L[i - j] for j in range(j0, j1 + 1))
        s += carry
        if s >= 1 << 64:
            raise BoundError(f"{name}: column {i} may reach {s.bit_length()} bits ({a!r} x {b!r})")
        carry = s >> LB
    val = (a.val * b.val * P_OVER_R + 1) * UP  # (ab + m p) / R < ab/R + p
    out = normalized(val, name)
    return out


def mul_sum2(a: V, b: V, c: V, d: V, name="mul_sum2"):
    """fp_mul_sum2: a b + c d with one Montgomery reduction (three mad chains per column)."""
    _record("mul_sum2", name, a, b, c, d)
    carry = 0
    for i in range(2 * NL):
        j0 = 0 if i < NL else i - (NL - 1)
        j1 = i if i < NL else NL - 1
        s = sum(a.limbs[j] * b.limbs[i - j] + c.limbs[j] * d.limbs[i - j] for j in range(j0, j1 + 1))
        s += sum(LM * P_L[i - j] for j in range(j0, j1 + 1))
        s += carry
        if s >= 1 << 64:
            raise BoundError(f"{name}: column {i} may reach {s.bit_length()} bits")
        carry = s >> LB
    return normalized(((a.val * b.val + c.val * d.val) * P_OVER_R + 1) * UP, name)


def mul_sum3(a: V, b: V, c: V, d: V, e: V, f: V, name="mul_sum3"):
    """fp_mul_sum3: a b + c d + e f with one Montgomery reduction (four mad chains per column)."""
    _record("mul_sum3", name, a, b, c, d, e, f)
    carry = 0
    for i in range(2 * NL):
        j0 = 0 if i < NL else i - (NL - 1)
        j1 = i if i < NL else NL - 1
        s = sum(a.limbs[j] * b.limbs[i - j] + c.limbs[j] * d.limbs[i - j] + e.limbs[j] * f.limbs[i - j]
                for j in range(j0, j1 + 1))
        s += sum(LM * P_L[i - j] for j in range(j0, j1 + 1))
        s += carry
        if s >= 1 << 64:
            raise BoundError(f"{name}: column {i} may reach {s.bit_length()} bits")
        carry = s >> LB
    return normalized(((a.val * b.val + c.val * d.val + e.val * f.val) * P_OVER_R + 1) * UP, name)


def mul_add8sqr(a: V, b: V, c: V, name="mul_add8sqr"):
    """fp_mul_add8sqr: a b + 8 c^2 with one reduction; the c^2 half as a squaring (cross products
    c_j (16 c_k) once, squares c_j (8 c_j)), whose column sums equal those of c (8 c)."""
    _record("mul_add8sqr", name, a, b, c)
    if max(c.limbs) << 4 >= 1 << 32:
        raise BoundError(f"{name}: 16 c_k must fit 32 bits ({c!r})")
    c8 = V([x << 3 for x in c.limbs], c.val * 8 * UP, name + ".8c")
    carry = 0
    for i in range(2 * NL):
        j0 = 0 if i < NL else i - (NL - 1)
        j1 = i if i < NL else NL - 1
        s = sum(a.limbs[j] * b.limbs[i - j] + c.limbs[j] * c8.limbs[i - j] for j in range(j0, j1 + 1))
        s += sum(LM * P_L[i - j] for j in range(j0, j1 + 1))
        s += carry
        if s >= 1 << 64:
            raise BoundError(f"{name}: column {i} may reach {s.bit_length()} bits")
        carry = s >> LB
    return normalized(((a.val * b.val + 8 * c.val * c.val) * P_OVER_R + 1) * UP, name)


def sqr(a: V, name="sqr"):
    """fp_sqr: same column sums as mul(a, a); the doubled operand 2 a_k must fit 32 bits."""
    if max(a.limbs) >= 1 << 31:
        raise BoundError(f"{name}: squaring input limb >= 2^31 ({a!r})")
    _record("sqr", name, a)
    return mul(a, a, name)  # recorded as a mul site too: the squaring's column bound IS mul(a, a)'s


def add_nr(a, b, name="add"):
    return V([x + y for x, y in zip(a.limbs, b.limbs)], (a.val + b.val) * UP, name)


def shl(a, s, name="shl"):
    return V([x << s for x in a.limbs], a.val * (1 << s) * UP, name)


def mul3(a, name="mul3"):
    return V([3 * x for x in a.limbs], a.val * 3 * UP, name)


def subk(a, b, kname, name="subk"):
    k = C[kname]
    for i in range(NL):
        if k[i] < b.limbs[i]:
            raise BoundError(f"{name}: {kname}[{i}] = {k[i]:#x} < subtrahend limb bound {b.limbs[i]:#x} ({b!r})")
    kv = const(k).val
    return V([x + y for x, y in zip(a.limbs, k)], (a.val + kv) * UP, name)


def norm(a, name="norm"):
    for l in a.limbs:
        if l + 16 >= 1 << 32:
            raise BoundError(f"{name}: norm input limb too large")
    return normalized(a.val, name)


def half(a, name="half"):
    """fp_half: a normalized (limbs below the top < 2^28); + p if odd (the top limb absorbs the
    carry), then one right shift across the limbs: normalized, value (v + 1) / 2."""
    if any(l > LM for l in a.limbs[: NL - 1]):
        raise BoundError(f"{name}: input not normalized {a!r}")
    if a.limbs[NL - 1] + P_L[NL - 1] + 1 >= 1 << 32:
        raise BoundError(f"{name}: top limb + p may overflow {a!r}")
    return normalized((a.val + 1) / 2 * UP, name)


def canon_ok(a, name="canon"):
    """fp_canon / fp_is_zero precondition: limbs < 2^32 - 16 (fp_norm), value < 256 p."""
    if max(a.limbs) >= (1 << 32) - 16 or a.val >= 256:
        raise BoundError(f"{name}: canon precondition violated {a!r}")


def reduce_once_ok(a, name="reduce_once"):
    """fp_reduce_once precondition: normalized, value < 2 p."""
    if any(l > LM for l in a.limbs) or a.val >= 2:
        raise BoundError(f"{name}: one conditional subtraction cannot canonicalize {a!r}")


def from_mont_ok(a, name="from_mont"):
    """fp_from_mont: a must be normalized (a < R); mul(a, 1) < p + 1 then reduce_once."""
    if any(l > LM for l in a.limbs):
        raise BoundError(f"{name}: input not normalized {a!r}")
    reduce_once_ok(mul(a, normalized(Fraction(1, 10**9)), name), name)


# ------------------------------------------------------------------------------------------
# Fp2 (components share bounds: one V per component pair, conservatively the join)
class V2:
    def __init__(self, c0, c1):
        self.c0, self.c1 = c0, c1


# ------------------------------------------------------------------------------------------
# bound sets: join / inflate / within on a V or a V2, and the one closed-set search
def join(*vs):
    """the least bound above all of vs"""
    if isinstance(vs[0], V2):
        return V2(join(*(v.c0 for v in vs)), join(*(v.c1 for v in vs)))
    return V([max(x) for x in zip(*(v.limbs for v in vs))], max(v.val for v in vs), "join")


def inflate(a, f=1.01):
    if isinstance(a, V2):
        return V2(inflate(a.c0, f), inflate(a.c1, f))
    limbs = list(a.limbs)
    limbs[NL - 1] = int(limbs[NL - 1] * f) + 2  # the top limb tracks the value
    return V(limbs, a.val * f + 0.01)


def within(a, b):
    """a subset of b (all bounds of a <= those of b)."""
    if isinstance(a, V2):
        return within(a.c0, b.c0) and within(a.c1, b.c1)
    return all(x <= y for x, y in zip(a.limbs, b.limbs)) and a.val <= b.val


def closed_set(start, step, rounds=12):
    """A bound set S (a tuple of V / V2) that contains `start` and is CLOSED under `step(*S) -> tuple` —
    hence bounds every state reached from start by any number of steps, for any input. Found by
    `rounds` joined iterations and one inflation (rounds = 0: from start as it is), then verified
    closed, a failing candidate joined with its image and inflated, 40 times at the most."""
    def grown(S):
        return tuple(join(s, t) for s, t in zip(S, step(*S)))

    S = tuple(start)
    if rounds:
        for _ in range(rounds):
            S = grown(S)
        S = tuple(inflate(s) for s in S)
    for _ in range(40):
        T = grown(S)
        if all(within(t, s) for t, s in zip(T, S)):
            return S
        S = tuple(inflate(t) for t in T)
    raise BoundError("bound set is not closed: values keep growing")


def ladder_set(start, dbl, madd):
    """closed_set for a ladder accumulator (X, Y, Z): one step is dbl, then optionally madd(base)"""
    def step(*S):
        d = dbl(*S)
        return tuple(join(a, b) for a, b in zip(d, madd(*d)))

    return closed_set(start, step)


def reduced(name=""):
    return normalized(2 - 1e-7, name)  # strictly below 2p (integers: at most 2p - 1)


def check_reduced(a, name):
    if a.val > 2 + 1e-6 or any(l > LM for l in a.limbs[: NL - 1]) or a.limbs[NL - 1] > reduced().limbs[NL - 1]:
        raise BoundError(f"{name}: expected a reduced (< 2p, normalized) value, got {a!r}")


def sub_red(a, b, name="sub_red"):
    """fp_sub_red: signed borrow chain a - b, + 2p if negative: reduced in, reduced out."""
    check_reduced(a, name), check_reduced(b, name)
    return reduced(name)


def add_red(a, b, name="add_red"):
    check_reduced(a, name), check_reduced(b, name)
    t = add_nr(a, b, name)
    if t.val >= 4 + 1e-6:
        raise BoundError(f"{name}: one conditional subtraction cannot reduce {t!r}")
    norm(t, name)
    return reduced(name)


def f2_mul(a: V2, b: V2, name="f2mul"):
    """f_mul(fp2): c0 = REDC(a0 b0 + a1 (4p - b1)), c1 = REDC(a0 b1 + a1 b0)."""
    for c in (a.c0, a.c1, b.c0, b.c1):
        check_reduced(c, name)
    nb1 = subk(normalized(0), b.c1, "KB_4_28", name + ".nb1")
    c0 = mul_sum2(a.c0, b.c0, a.c1, nb1, name + ".c0")
    c1 = mul_sum2(a.c0, b.c1, a.c1, b.c0, name + ".c1")
    check_reduced(c0, name), check_reduced(c1, name)
    return V2(c0, c1)


def f2_sqr(a: V2, name="f2sqr"):
    check_reduced(a.c0, name), check_reduced(a.c1, name)
    s = add_nr(a.c0, a.c1)
    d = subk(a.c0, a.c1, "KB_4_28", name + ".d")
    t = shl(a.c0, 1)
    c0, c1 = mul(s, d, name + ".c0"), mul(t, a.c1, name + ".c1")
    check_reduced(c0, name), check_reduced(c1, name)
    return V2(c0, c1)


# ------------------------------------------------------------------------------------------
# formulas (mirror csrc/curve.hpp)
# ---- Fp, radix 2^28: the generic jac_madd / jac_eq_affine with F = fp and jac_dbl(jac<fp>&) — the
# reference-algorithm ladder in_subgroup_ref<fp>, the group FFT, the MSM and the generator. (The G1
# fast ladders run on radix 2^30: tests/f30_ladder_model.py.)
def jac_dbl(X, Y, Z):
    """jac_dbl(jac<fp>&) — the hot path (-Y3 = E (X3 - D) + 8 B^2 in one reduction, Y3 = K - that)."""
    a = sqr(X, "A")
    b = sqr(Y, "B")
    t = shl(X, 2)
    d = mul(t, b, "D")
    e = norm(mul3(a), "E")
    t = shl(Y, 1)
    z3 = mul(t, Z, "Z3")
    f = sqr(e, "F")
    t = shl(d, 1)
    x3 = subk(f, t, "KB_8_29", "X3")
    t = subk(f, mul3(d), "KB_8_30", "F-3D")
    ny3 = mul_add8sqr(e, t, b, "-Y3")
    y3 = subk(normalized(0), ny3, "KB_2_28", "Y3")
    return x3, y3, z3


def jac_madd(X, Y, Z, x2, y2):
    """jac_madd<fp>: the result joined with the equal-point branch (jac_dbl) and the Z1 = 0 branch
    (the base itself); the base (x2, y2) normalized."""
    z1z1 = sqr(Z, "Z1Z1")
    h = norm(subk(mul(x2, z1z1, "U2"), X, "KB_128_31", "H"))
    t = mul(mul(y2, Z, "y2Z"), z1z1, "S2")
    r = norm(subk(t, Y, "KB_64_31", "r'"))
    canon_ok(Z), canon_ok(h), canon_ok(r)
    xd, yd, zd = jac_dbl(X, Y, Z)  # the equal-point branch
    hh = sqr(h, "HH")
    z3 = mul(shl(Z, 1), h, "Z3")
    i = norm(shl(hh, 2))
    j = mul(h, i, "J")
    v = mul(X, i, "V")
    t = subk(shl(sqr(r, "r'^2"), 2), j, "KB_32_28", "X3a")
    x3 = norm(subk(t, shl(v, 1), "KB_64_29", "X3"))
    vx = norm(subk(v, x3, "KB_128_28", "V-X3"))
    nj = subk(normalized(0), j, "KB_4_28", "Y3.nd")  # f_mul_sub: r (V - X3) - 2 Y1 J, J negated against KB_4_28
    y3 = mul_sum2(shl(r, 1), vx, shl(Y, 1), nj, "Y3")
    return join(x3, xd, x2), join(y3, yd, y2), join(z3, zd, normalized(1))


def jac_eq_affine(X, Y, Z, x, y):
    z2 = sqr(Z, "z2")
    canon_ok(subk(mul(x, z2, "xZ2"), X, "KB_128_31", "eqx"))
    canon_ok(subk(mul(y, mul(z2, Z, "z3"), "yZ3"), Y, "KB_128_31", "eqy"))
    canon_ok(Z)


def ladder_invariant(base_x, base_y):
    """The bound set of the Y-form Fp ladder (in_subgroup_ref<fp>: ark's double-and-add), from (x, y, 1)."""
    return ladder_set((base_x, base_y, normalized(1)), jac_dbl, lambda *d: jac_madd(*d, base_x, base_y))


# ------------------------------------------------------------------------------------------
# Fp2 in the carry-free ("lazy") discipline of the G1 path — the G2 ladders (curve.hpp
# jac_dbl<W>(jac<fp2>&), jac_madd<W>(jac<fp2>&, ..), jac_tpl_affine_w(jac<fp2>&), jac_eq_affine(jac<fp2>, ..); W = false
# the Y form of in_subgroup_ref<fp2>, the FFT, the MSM and the generator, W = true the fast ladder's
# W = 2Y form). Each component is a V with its own limb / value bounds, exactly as for Fp.
def mul2(a: V2, b: V2, kname, name="mul2"):
    """f2_mul_lz: c0 = REDC(a0 b0 + a1 (K - b1)), c1 = REDC(a0 b1 + a1 b0)."""
    nb1 = subk(normalized(0), b.c1, kname, name + ".nb1")
    return V2(mul_sum2(a.c0, b.c0, a.c1, nb1, name + ".c0"), mul_sum2(a.c0, b.c1, a.c1, b.c0, name + ".c1"))


def sqr2(a: V2, kname, name="sqr2"):
    """f2_sqr_lz: c0 = REDC((a0 + a1)(a0 + K - a1)), c1 = REDC(2 a0 a1)."""
    s = add_nr(a.c0, a.c1, name + ".s")
    d = subk(a.c0, a.c1, kname, name + ".d")
    return V2(mul(s, d, name + ".c0"), mul(shl(a.c0, 1), a.c1, name + ".c1"))


def subk2(a, b, kname, name="subk2"):
    return V2(subk(a.c0, b.c0, kname, name + ".c0"), subk(a.c1, b.c1, kname, name + ".c1"))


def norm2(a, name="norm2"):
    return V2(norm(a.c0, name + ".c0"), norm(a.c1, name + ".c1"))


def shl2(a, s, name="shl2"):
    return V2(shl(a.c0, s, name), shl(a.c1, s, name))


def mul3_2(a, name="mul3_2"):
    return V2(mul3(a.c0, name), mul3(a.c1, name))


def zero_ok2(a, name):
    canon_ok(a.c0, name), canon_ok(a.c1, name)


def add2(a, b, name="add2"):
    return V2(add_nr(a.c0, b.c0, name), add_nr(a.c1, b.c1, name))


def jac_eq_affine_fp2(X, Y, Z, x, y):
    """curve.hpp jac_eq_affine(const jac<fp2>&, ..): x Z^2 == X, y Z^3 == Y, Z != 0."""
    z2 = sqr2(Z, "KB_16_28", "z2")
    t = subk2(mul2(x, z2, "KB_2_28", "xZ2"), X, "KB_32_28", "eqx")
    zero_ok2(t, "eqx")
    z3 = mul2(z2, Z, "KB_16_28", "z3")
    t = subk2(mul2(y, z3, "KB_2_28", "yZ3"), Y, "KB_32_29", "eqy")
    zero_ok2(t, "eqy")
    zero_ok2(Z, "Z")


def jac_tpl_affine_fp2_w(x, w):
    """jac_tpl_affine_w(jac<fp2>&): the scaled triple (X3/4, W3/8, E) from (x, w = 2y):
    YYw = w^2, T = YYw^2, E = 3 x YYw - MM, X3/4 = x EE - YYw U, W3/8 = w (U (T - U) - E EE)."""
    xx = sqr2(x, "KB_2_28", "XX")
    yyw = sqr2(w, "KB_4_29", "YYw")
    t = sqr2(yyw, "KB_2_28", "T")
    m = norm2(mul3_2(xx), "M")
    mm = sqr2(m, "KB_4_28", "MM")
    e = norm2(subk2(mul3_2(mul2(x, yyw, "KB_2_28", "x YYw")), mm, "KB_2_28", "3 x YYw - MM"), "E")
    ee = sqr2(e, "KB_16_28", "EE")
    s2 = sqr2(norm2(add2(m, e), "M+E"), "KB_32_28", "S2")
    u = subk2(subk2(subk2(s2, mm, "KB_2_28", "S2-MM"), ee, "KB_4_28", "-EE"), t, "KB_2_28", "-T")
    u = norm2(u, "U")
    a = mul2(x, ee, "KB_2_28", "xEE")
    b = mul2(yyw, u, "KB_64_28", "YYwU")
    x3 = norm2(subk2(a, b, "KB_2_28", "xEE-YYwU"), "X3/4")
    c = mul2(u, norm2(subk2(t, u, "KB_64_28", "T-U"), "T-U"), "KB_128_28", "U(T-U)")
    d = mul2(e, ee, "KB_2_28", "E EE")
    inner = norm2(subk2(c, d, "KB_2_28", "inner"), "inner")
    w3 = mul2(w, inner, "KB_8_28", "W3/8")
    return x3, w3, e


def jac_dbl_fp2(X, Y, Z, w=False):
    """curve.hpp jac_dbl<W>(jac<fp2>&): X, Y, Z normalized in, normalized out. w: Y is W = 2Y (limbs to 2^29)."""
    if w:
        b = sqr2(Y, "KB_32_29", "B'")                       # B' = W^2: the constant against W
        z3 = mul2(Y, Z, "KB_16_28", "Z3")                   # Z3 = W Z
    else:
        b = sqr2(Y, "KB_32_28", "B")
        z3 = mul2(shl2(Y, 1), Z, "KB_16_28", "Z3")
    a = sqr2(X, "KB_16_28", "A")
    d = mul2(X if w else shl2(X, 2), b, "KB_2_28", "D")     # D = X B' = 4 X B
    e = norm2(mul3_2(a), "E")
    f = sqr2(e, "KB_4_28", "F")
    x3 = norm2(subk2(f, shl2(d, 1), "KB_4_29", "X3"), "X3")
    t = subk2(d, x3, "KB_8_28", "D-X3")
    u = subk(normalized(0), t.c1, "KB_16_30", "-t1")
    s = add_nr(b.c0, b.c1, "b0+b1")
    if w:  # W3 = (2E) t - B'^2: the factors of B'^2 unscaled
        e = shl2(e, 1, "2E")
        n0 = norm(subk(b.c1, b.c0, "KB_2_28", "b1-b0"), "b1-b0")
        n1 = subk(normalized(0), b.c1, "KB_2_28", "-b1")
    else:  # Y3 = E t - 8 B^2: the negated factors scaled by 8, normalized
        n0 = norm(subk(normalized(0), shl(norm(subk(b.c0, b.c1, "KB_2_28", "b0-b1")), 3), "KB_64_31", "-8(b0-b1)"))
        n1 = norm(subk(normalized(0), shl(b.c1, 3), "KB_16_31", "-8b1"))
    y0 = mul_sum3(e.c0, t.c0, e.c1, u, s, n0, "Y3.c0")
    y1 = mul_sum3(e.c0, t.c1, e.c1, t.c0, shl(b.c0, 1), n1, "Y3.c1")
    return x3, V2(y0, y1), z3


def jac_madd_fp2(X, Y, Z, x2, y2, w=False):
    """curve.hpp jac_madd<W>(jac<fp2>&, ..): normalized in / out; the base (x2, y2) normalized (w: y2 = 2y). The
    result joined with the equal-point branch (jac_dbl_fp2) and the Z1 = 0 branch (the base, Z = 1)."""
    z1z1 = sqr2(Z, "KB_16_28", "Z1Z1")
    u2 = mul2(x2, z1z1, "KB_2_28", "U2")
    h = norm2(subk2(u2, X, "KB_32_28", "H"), "H")
    t = mul2(y2, Z, "KB_16_28", "y2Z")
    s2 = mul2(t, z1z1, "KB_2_28", "S2")
    r = norm2(subk2(s2, Y, "KB_32_29" if w else "KB_32_28", "r"), "r")  # w: r = 2 S2 - W1 is ark's r; else r' = r / 2
    zero_ok2(Z, "Z"), zero_ok2(h, "H"), zero_ok2(r, "r")
    xd, yd, zd = jac_dbl_fp2(X, Y, Z, w)  # the equal-point branch
    hh = sqr2(h, "KB_64_28", "HH")
    z3 = mul2(shl2(Z, 1), h, "KB_64_28", "Z3m")
    i = shl2(hh, 2, "I")
    j = mul2(h, i, "KB_8_30", "J")
    v = mul2(X, i, "KB_8_30", "V")
    rr = sqr2(r, "KB_64_28", "r^2")
    if not w:
        rr = shl2(rr, 2)                                   # r^2 = 4 r'^2
    x3 = subk2(rr, j, "KB_2_28", "X3a")
    x3 = norm2(subk2(x3, shl2(v, 1), "KB_4_29", "X3m"), "X3m")
    vx = subk2(v, x3, "KB_32_28", "V-X3")
    a = mul2(shl2(r, 1), vx, "KB_64_30", "r(V-X3)")
    b = mul2(shl2(Y, 1), j, "KB_2_28", "2Y1J")
    y3 = norm2(subk2(a, b, "KB_4_28", "Y3m"), "Y3m")
    one = V2(normalized(1), normalized(1))
    return join(x3, xd, x2), join(y3, yd, y2), join(z3, zd, one)


def ladder_invariant_fp2(base_x, base_y, w=False):
    """The bound set of a G2 ladder: the Y form from (x, y, 1) (in_subgroup_ref<fp2>), or with w the
    fast ladder's W form from its opening tripling (mul_abs_u_affine<fp2>; base_y = 2y)."""
    start = jac_tpl_affine_fp2_w(base_x, base_y) if w else (base_x, base_y, V2(normalized(1), normalized(0)))
    return ladder_set(start, lambda *S: jac_dbl_fp2(*S, w), lambda *d: jac_madd_fp2(*d, base_x, base_y, w))
