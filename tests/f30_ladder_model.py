"""Exact model and bound calculus of the G1 subgroup ladders on the radix-2^30 core
(csrc/fp381.hpp f30_mul_sum2 / f30_mul_addsqr / f30_norm / f30_is_zero and the digit-wise forms;
csrc/curve.hpp jac_dbl_w / jac_madd_w / jac_tpl_affine_w / jac_eq_affine for jac<f30>).

A value V carries its exact digits (13 Python integers, or None for a bounds-only run) and a bound
B = (d, top, v): |lower digit| <= d, |top digit| <= top, |value| <= v. Every function below

  * computes the device function step by step on the digits, with every 64-bit accumulator checked
    against int64 and every 32-bit result against int32;
  * derives the output bound from the INPUT BOUNDS alone, and proves the function's precondition
    from them: for the products, that the sum of absolute values of every column (the actual digits
    of p, |m_i| <= 2^29, the carry, the bias) stays below 2^63 for every input within the bounds;
  * asserts the exact digits lie within the derived bound.

So one bounds-only run of a formula proves it for every input inside its input bounds, and the
exact runs check the bound derivations and the arithmetic. tests/test_f30_ladder.py drives both.
"""
import field_bounds_model

P = field_bounds_model.FIELDS["bls12_381"][0]
HDR = field_bounds_model.load_consts()  # bls12_381_consts.hpp, by name
N = 13
M30 = (1 << 30) - 1
R30 = 1 << 390
ABS_U = HDR["BLS_ABS_U"]
ZK = 16  # curve.hpp F30_ZK
P30, PINV30 = HDR["P30"], HDR["PINV30"]
LOW = sum(1 << (30 * k) for k in range(N - 1))  # value of the lower digits, all 1


def val(d):
    return sum(v << (30 * k) for k, v in enumerate(d))


def digits(x):
    """x (any sign) as 12 balanced digits in [-2^29, 2^29) and a top digit that takes the rest"""
    out = []
    for _ in range(N - 1):
        d = sext(x, 30)
        out.append(d)
        x = (x - d) >> 30
    return out + [x]


def sext(x, bits):
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def s64(x, what):
    if not -(1 << 63) <= x < (1 << 63):
        raise OverflowError(f"{what}: {x:#x} leaves int64")
    return x


def s32(x, what):
    if not -(1 << 31) <= x < (1 << 31):
        raise OverflowError(f"{what}: {x:#x} leaves int32")
    return x


class B:
    """-d <= lower digit <= pos (pos <= d; a product's digits are < 2^29, which 3 x (a product)
    needs to fit f30_norm), |top digit| <= top, |value| <= v"""

    def __init__(self, d, top, v, pos=None):
        self.d, self.top, self.v = d, top, v
        self.pos = d if pos is None else pos

    def dig(self, k):
        return self.top if k == N - 1 else self.d

    def join(self, o):
        return B(max(self.d, o.d), max(self.top, o.top), max(self.v, o.v), max(self.pos, o.pos))

    def within(self, o):
        return self.d <= o.d and self.top <= o.top and self.v <= o.v and self.pos <= o.pos

    def __repr__(self):
        return f"B(d=2^29+{self.d - (1 << 29)}, top={self.top}, v={self.v / P:.3f}p)"


class V:
    def __init__(self, d, b):
        self.d, self.b = d, b
        if d is not None:
            assert len(d) == N
            assert all(-b.d <= x <= b.pos for x in d[:-1]), (d, b)
            assert abs(d[-1]) <= b.top, (d[-1], b)
            assert abs(val(d)) <= b.v, (val(d) / P, b)
        assert b.d < 1 << 31 and b.top < 1 << 31, f"digit bound leaves int32: {b}"


def top_from_value(v, d):
    """|top digit| of a value |x| <= v whose lower digits are bounded by d"""
    return (v + d * LOW) >> 360


def of_int(x, v=None):
    """a balanced value (f30_from_fp's output) of the integer x, |x| <= v"""
    v = abs(x) if v is None else v
    return V(digits(x), B(1 << 29, top_from_value(v, 1 << 29) + 1, v))


def bound_only(b):
    return V(None, b)


# ------------------------------------------------------------------------------- products
def _check_columns(pairs, what):
    """sum of |products| per column for operand bounds `pairs` = [(Ba, Bb), ...], + |m| |p| + carry
    + bias < 2^63 — the precondition of the device scan, for every input within the bounds"""
    carry = 0
    worst = 0
    for i in range(2 * N - 1):
        j0 = 0 if i < N else i - (N - 1)
        j1 = i if i < N else N - 1
        tot = carry + (1 << 29)
        for a, b in pairs:
            tot += sum(a.dig(j) * b.dig(i - j) for j in range(j0, j1 + 1))
        tot += sum((1 << 29) * abs(P30[i - j]) for j in range(j0, j1 + 1))
        worst = max(worst, tot)
        carry = (tot >> 30) + 1
    if worst >= 1 << 63:
        raise OverflowError(f"{what}: worst-case column 2^{worst.bit_length()} for {pairs}")
    return worst


def _scan(prods, sqrs):
    """The device column scan on exact digits: prods = [(a, b), ...] full products, sqrs = [c, ...]
    squares computed as cross products once (c_j * 2 c_k) plus the diagonal. A lower column's a_i b_0
    is the last product INSIDE the column's run, before the m p products, as in the device's serial
    run (f30_mul puts it at x[n] of the one statement); tests/test_fp30.py drives this scan too."""
    m = [0] * N
    r = [0] * N
    acc = 0
    for i in range(2 * N - 1):
        j0 = 0 if i < N else i - (N - 1)
        j1 = i - 1 if i < N else N - 1
        col = 0 if i < N else 1 << 29
        for a, b in prods:
            for j in range(j0, j1 + 1):
                col = s64(col + a[j] * b[i - j], "ab")
            if i < N:
                col = s64(col + a[i] * b[0], "ab")
        for c in sqrs:
            c2 = [s32(2 * x, "2c") for x in c]
            for j in range(j0, i):
                if 2 * j < i and i - j < N:
                    col = s64(col + c[j] * c2[i - j], "cc")
            if i % 2 == 0:
                col = s64(col + c[i // 2] * c[i // 2], "cc")
        accp = 0
        for j in range(j0, j1 + 1):
            accp = s64(accp + m[j] * P30[i - j], "mp")
        acc = s64(acc + col, "acc")
        acc = s64(acc + accp, "acc")
        if i < N:
            m[i] = sext((acc & 0xFFFFFFFF) * PINV30, 30)
            acc = s64(acc + m[i] * P30[0], "acc")
            assert acc % (1 << 30) == 0
        else:
            r[i - N] = (acc & M30) - (1 << 29)
        acc >>= 30
    r[N - 1] = s32(acc, "top")
    return r


def _product(prods, sqrs, what):
    pairs = [(a.b, b.b) for a, b in prods] + [(c.b, c.b) for c in sqrs]
    _check_columns(pairs, what)
    num = sum(a.v * b.v for a, b in pairs)
    # r R30 = sum + m p with |m| <= 2^29 (R30 - 1) / (2^30 - 1)
    v = num // R30 + P // 2 + (P >> 29) + 2
    out = B(1 << 29, top_from_value(v, 1 << 29) + 1, v, (1 << 29) - 1)
    if any(x.d is None for pr in prods for x in pr) or any(c.d is None for c in sqrs):
        return V(None, out)
    r = _scan([(a.d, b.d) for a, b in prods], [c.d for c in sqrs])
    want = sum(val(a.d) * val(b.d) for a, b in prods) + sum(val(c.d) ** 2 for c in sqrs)
    assert (val(r) * R30 - want) % P == 0, what
    return V(r, out)


def mul(a, b):
    return _product([(a, b)], [], "f30_mul")


def sqr(a):
    return _product([], [a], "f30_sqr")


def mul_sum2(a, b, c, d):
    return _product([(a, b), (c, d)], [], "f30_mul_sum2")


def mul_addsqr(a, b, c):
    return _product([(a, b)], [c], "f30_mul_addsqr")


# ------------------------------------------------------------------------------- digit-wise
def _lin(terms, what):
    """sum of k * x over terms [(k, x), ...], digit-wise in int32"""
    b = B(max(sum(k * x.b.d if k > 0 else -k * x.b.pos for k, x in terms),
              sum(k * x.b.pos if k > 0 else -k * x.b.d for k, x in terms)),
          sum(abs(k) * x.b.top for k, x in terms), sum(abs(k) * x.b.v for k, x in terms),
          sum(k * x.b.pos if k > 0 else -k * x.b.d for k, x in terms))
    if any(x.d is None for _, x in terms):
        return V(None, b)
    return V([s32(sum(k * x.d[i] for k, x in terms), what) for i in range(N)], b)


def add(a, b):
    return _lin([(1, a), (1, b)], "add")


def sub(a, b):
    return _lin([(1, a), (-1, b)], "sub")


def neg(a):
    return _lin([(-1, a)], "neg")


def dbl(a):
    return _lin([(2, a)], "dbl")


def mul3(a):
    return _lin([(3, a)], "mul3")


def norm(a, s=0):
    """f30_norm<S>: 2^S a, every digit at once; a_k + 2^(29-S) must stay inside int32"""
    assert a.b.pos + (1 << (29 - s)) < 1 << 31 and a.b.d <= 1 << 31, f"f30_norm<{s}> input digit bound {a.b}"
    cmax = (a.b.d + (1 << (29 - s))) >> (30 - s)
    b = B((1 << 29) + cmax, (a.b.top << s) + cmax, a.b.v << s)
    if a.d is None:
        return V(None, b)
    r, c = [], 0
    for k in range(N - 1):
        lo = sext(a.d[k], 30 - s)
        cn = s32(a.d[k] + (1 << (29 - s)), "norm") >> (30 - s)
        r.append(s32((lo << s) + c, "norm"))
        c = cn
    r.append(s32((a.d[N - 1] << s) + c, "norm top"))
    assert val(r) == val(a.d) << s
    return V(r, b)


def is_zero(a, k_max=ZK):
    """f30_is_zero<K>: exact for |value| <= K p, any int32 digits"""
    assert a.b.v <= k_max * P, f"zero test on a value beyond {k_max} p: {a.b}"
    if a.d is None:
        return None
    k = sext((a.d[0] & 0xFFFFFFFF) * ((-PINV30) & 0xFFFFFFFF), 30)
    if not -k_max <= k <= k_max:
        return False
    c, diff = 0, 0
    for i in range(N):
        c = s64(c + a.d[i] - k * P30[i], "is_zero")
        if i < N - 1:
            diff |= c & M30
            c >>= 30
    return diff == 0 and c == 0


# ------------------------------------------------------------------------------- curve.hpp, jac<f30>
def one():
    return of_int(R30 % P)


def jac_dbl_w(X, W, Z):
    a = sqr(X)
    b = sqr(W)
    d = mul(X, b)
    e = norm(mul3(a))
    z3 = mul(W, Z)
    f = sqr(e)
    x3 = norm(sub(f, dbl(d)))
    t = norm(sub(x3, d), 1)
    w3 = neg(mul_addsqr(e, t, b))
    return x3, w3, z3


def jac_tpl_affine_w(x, w):
    xx = sqr(x)
    yy = sqr(w)
    t = sqr(yy)
    m = norm(mul3(xx))
    mm = sqr(m)
    s = norm(mul3(mul(x, yy)))
    e = norm(sub(s, mm))
    ee = sqr(e)
    s = sqr(norm(add(m, e)))
    s = norm(sub(s, mm))
    s = norm(sub(s, ee))
    u = norm(sub(s, t))
    x3 = norm(mul_sum2(x, ee, yy, neg(u)), 2)
    t = norm(sub(t, u))
    s = mul_sum2(u, t, e, neg(ee))
    w3 = norm(mul(w, s), 3)
    z3 = norm(e, 1)
    return x3, w3, z3


def jac_madd_w(X, W, Z, x2, w2, decide=True):
    """decide=False: a bounds-only run of the general branch"""
    z1z1 = sqr(Z)
    h = norm(sub(mul(x2, z1z1), X))
    r = norm(sub(mul(mul(w2, Z), z1z1), W))
    z1zero, hz, rz = is_zero(Z), is_zero(h), is_zero(r)
    if decide and z1zero:
        return x2, w2, one()
    if decide and hz and rz:
        return jac_dbl_w(X, W, Z)
    hh = sqr(h)
    z3 = mul(dbl(Z), h)
    i4 = norm(hh, 2)
    j = mul(h, i4)
    v = mul(X, i4)
    t = norm(sub(sub(sqr(r), j), v))
    x3 = norm(sub(t, v))
    vx = norm(sub(v, x3))
    w3 = mul_sum2(norm(r, 1), vx, norm(W, 1), neg(j))
    return x3, w3, z3


def mul_abs_u_affine(x, w, trace=None):
    X, W, Z = jac_tpl_affine_w(x, w)
    for b in range(ABS_U.bit_length() - 3, -1, -1):
        X, W, Z = jac_dbl_w(X, W, Z)
        if (ABS_U >> b) & 1:
            X, W, Z = jac_madd_w(X, W, Z, x, w)
        if trace is not None:
            trace.append((X, W, Z))
    return X, W, Z


def jac_eq_affine(X, W, Z, x, w):
    z2 = sqr(Z)
    ok = is_zero(sub(mul(x, z2), X))
    ok2 = is_zero(sub(mul(w, mul(z2, Z)), W))
    return ok and ok2 and not is_zero(Z)


def in_subgroup_fast_g1(x, w):
    """x, w = 2y balanced R30 forms (g1_park_base); BETA30 from the header"""
    q1 = mul_abs_u_affine(x, w)
    X, W, Z = mul_abs_u_affine(q1[0], q1[1])
    Z = mul(Z, q1[2])
    return jac_eq_affine(X, W, Z, mul(x, of_int(val(HDR["BETA30"]))), neg(w))


# ------------------------------------------------------------------------------- 14 x 28 <-> 13 x 30
# fp381.hpp f30_from_mont<H> / fp_mont_from_f30<H> (the parked base point; codec_parts.hpp
# g1_park_base and g1_in_subgroup's reference-ladder path), limb by limb
M28 = (1 << 28) - 1
P28 = [(P >> (28 * k)) & M28 for k in range(13)] + [P >> 364]


def limbs28(x):
    return [(x >> (28 * k)) & M28 for k in range(13)] + [x >> 364]


def val28(l):
    return sum(v << (28 * k) for k, v in enumerate(l))


def u32(x, what):
    if not 0 <= x < 1 << 32:
        raise OverflowError(f"{what}: {x:#x} leaves uint32")
    return x


def fp_half(a):
    """fp_half: a normalized; + p if odd, one right shift across the limbs"""
    odd = a[0] & 1
    t, c = [], 0
    for i in range(13):
        s = u32(a[i] + (P28[i] if odd else 0) + c, "half")
        t.append(s & M28)
        c = s >> 28
    t.append(u32(a[13] + (P28[13] if odd else 0) + c, "half top"))
    return [(t[i] >> 1) | ((t[i + 1] & 1) << 27) for i in range(13)] + [t[13] >> 1]


def f30_from_fp(n):
    """f30_from_fp of normalized limbs (fp_half's output): the same integer, balanced digits"""
    r, c = [], 0
    for k in range(N):
        bit = 30 * k
        i, off = bit // 28, bit % 28
        u = ((n[i] >> off) | ((n[i + 1] << (28 - off)) if i + 1 < 14 else 0)) & 0xFFFFFFFF
        if k < N - 1:
            t = (u & M30) + c
            c = (t + (1 << 29)) >> 30
            r.append(sext(t, 30))
        else:
            r.append(s32(u + c, "from_fp top"))
    return r


def from_mont(h, a):
    """f30_from_mont<H>: a = normalized R = 2^392 limbs, value < 1.001 p; out: a balanced V, value in
    [0, 1.001 p), of the integer a / 2^H mod p"""
    assert val28(a) < P + P // 1000 and all(x <= M28 for x in a[:13])
    t = fp_half(a)
    if h == 2:
        t = fp_half(t)
    r = f30_from_fp(t)
    assert val(r) == val28(t) and (val(r) << h) % P == val28(a) % P and val(r) < P + P // 1000
    v = P + P // 1000
    return V(r, B(1 << 29, top_from_value(v, 1 << 29) + 1, v, (1 << 29) - 1))


def fp_from_f30(z):
    """fp_from_f30 for z > -p: + p, unsigned digits, 28-bit limbs, one conditional subtraction"""
    u, c = [], 0
    for k in range(N):
        t = s32(z[k] + P30[k] + c, "from_f30")
        if k < N - 1:
            u.append(t & M30)
            c = t >> 30
        else:
            assert t >= 0
            u.append(t)
    limbs = []
    for j in range(14):
        bit = 28 * j
        i, off = bit // 30, bit % 30
        v = u[i] >> off
        if off > 2 and i + 1 < N:
            v |= (u[i + 1] << (30 - off)) & 0xFFFFFFFF
        limbs.append(v & M28 if j < 13 else v)
    x = val28(limbs)
    assert x == val(z) + P
    return limbs28(x - P if x >= P else x)


def mont_from_f30(h, z):
    """fp_mont_from_f30<H>: z a V with value in [0, 1.001 p); out: normalized limbs, value < 1.01 p,
    of 2^H z mod p (each step fp_add + fp_norm + one conditional subtraction of p)"""
    assert 0 <= val(z.d) < P + P // 1000
    r = fp_from_f30(z.d)
    for _ in range(h):
        x = val28([u32(2 * l, "dbl") for l in r])
        r = limbs28(x - P if x >= P else x)
    assert val28(r) % P == (val(z.d) << h) % P and val28(r) < P + P // 100
    assert all(l <= M28 for l in r[:13])
    return r
