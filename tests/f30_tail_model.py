"""Exact model and bound calculus of the radix-2^30 scans' TAIL forms (csrc/fp381.hpp f30_mul<K0, K1> /
f30_sqr<K0, K1>, f30_column, f30_top) and of the G1 subgroup ladders that use them (csrc/curve.hpp
jac_dbl_w / jac_madd_w / jac_tpl_affine_w for jac<f30>), on the primitives of f30_ladder_model.py.

A tail (K, t) puts K t_k into upper column 13 + k of a product's scan before that column's digit is
taken, and K t_12 onto the top digit, so the scan returns the balanced digits of

    V + sum K val(t),     V = (a b + m p) / 2^390 the integer the plain form spells out,

where the plain form was followed by a digit-wise difference and an f30_norm. As in
f30_ladder_model.py every function computes the device function step by step on exact digits (every
64-bit accumulator checked against int64, in the device's order: the lane products, the m p
products, the tails), derives its output bound from the INPUT BOUNDS alone and proves its
precondition from them: the worst-case column, the tails' |K| |t_k| included, below 2^63.
f30_ladder_model.py's own jac_* functions describe the forms without tails, which the device ran
before; tests/test_f30_tail.py checks these against them value for value."""
import f30_ladder_model as M
from f30_ladder_model import B, N, P, P30, PINV30, M30, R30, V, s32, s64, sext, val

K_MIN, K_MAX = -16, 64  # a tail's factor is an inline constant of the mad


# ------------------------------------------------------------------------------- the tail scan
def check_columns(pairs, tails, what):
    """f30_ladder_model._check_columns with the tails [(K, B), ...] in the upper columns: the sum of
    absolute values of every column stays below 2^63 for every input within the bounds. Returns the
    worst column sum."""
    carry = 0
    worst = 0
    for i in range(2 * N - 1):
        j0 = 0 if i < N else i - (N - 1)
        j1 = i if i < N else N - 1
        tot = carry + (1 << 29)
        for a, b in pairs:
            tot += sum(a.dig(j) * b.dig(i - j) for j in range(j0, j1 + 1))
        tot += sum((1 << 29) * abs(P30[i - j]) for j in range(j0, j1 + 1))
        if i >= N:
            tot += sum(abs(k) * t.dig(i - N) for k, t in tails)
        worst = max(worst, tot)
        carry = (tot >> 30) + 1
    if worst >= 1 << 63:
        raise OverflowError(f"{what}: worst-case column 2^{worst.bit_length()} for {pairs} + {tails}")
    return worst


def scan(prods, sqrs, tails=(), stats=None):
    """The device column scan on exact digits (f30_ladder_model._scan, the same order of accumulation)
    with tails [(K, digits), ...]: in an upper column the tails' mads follow the m p products on the
    running accumulator, then the digit is taken; the top digit is the last carry + sum K t_12.
    stats: a dict that receives "peak", the largest |column sum| met."""
    m = [0] * N
    r = [0] * N
    acc = 0
    peak = 0
    for i in range(2 * N - 1):
        j0 = 0 if i < N else i - (N - 1)
        j1 = i - 1 if i < N else N - 1
        for a, b in prods:
            for j in range(j0, j1 + 1):
                acc = s64(acc + a[j] * b[i - j], "ab")
            if i < N:
                acc = s64(acc + a[i] * b[0], "ab")
        for c in sqrs:
            c2 = [s32(2 * x, "2c") for x in c]
            for j in range(j0, i):
                if 2 * j < i and i - j < N:
                    acc = s64(acc + c[j] * c2[i - j], "cc")
            if i % 2 == 0:
                acc = s64(acc + c[i // 2] * c[i // 2], "cc")
        for j in range(j0, j1 + 1):
            acc = s64(acc + m[j] * P30[i - j], "mp")
        if i < N:
            peak = max(peak, abs(acc))
            m[i] = sext((acc & 0xFFFFFFFF) * PINV30, 30)
            acc = s64(acc + m[i] * P30[0], "acc")
            assert acc % (1 << 30) == 0
            acc >>= 30
        else:
            for k, t in tails:
                acc = s64(acc + k * t[i - N], "tail")
            peak = max(peak, abs(acc))
            r[i - N] = sext(acc, 30)
            acc = s64(acc + (1 << 29), "carry") >> 30
    top = s32(acc, "top carry")
    for k, t in tails:
        top = s32(top + s32(k * t[N - 1], "top tail"), "top")
    r[N - 1] = top
    if stats is not None:
        stats["peak"] = peak
    return r


def product_tail(prods, sqrs, tails, what):
    """tails = [(K, V), ...], at most two. Out: digits in [-2^29, 2^29) below the top, value
    V + sum K val(t) with |V| bounded as the plain form's."""
    assert len(tails) <= 2 and all(K_MIN <= k <= K_MAX and k != 0 for k, _ in tails), what
    pairs = [(a.b, b.b) for a, b in prods] + [(c.b, c.b) for c in sqrs]
    worst = check_columns(pairs, [(k, t.b) for k, t in tails], what)
    num = sum(a.v * b.v for a, b in pairs)
    v = num // R30 + P // 2 + (P >> 29) + 2 + sum(abs(k) * t.b.v for k, t in tails)
    out = B(1 << 29, M.top_from_value(v, 1 << 29) + 1, v, (1 << 29) - 1)
    assert out.top < 1 << 31, f"{what}: top digit bound leaves int32"
    ops = [x for pr in prods for x in pr] + list(sqrs) + [t for _, t in tails]
    if any(x.d is None for x in ops):
        r = V(None, out)
    else:
        d = scan([(a.d, b.d) for a, b in prods], [c.d for c in sqrs], [(k, t.d) for k, t in tails])
        want = sum(val(a.d) * val(b.d) for a, b in prods) + sum(val(c.d) ** 2 for c in sqrs)
        lin = sum(k * val(t.d) for k, t in tails)
        assert ((val(d) - lin) * R30 - want) % P == 0, what
        r = V(d, out)
    r.worst = worst
    return r


def mul_tail(a, b, *tails):
    return product_tail([(a, b)], [], list(tails), "f30_mul tail")


def sqr_tail(a, *tails):
    return product_tail([], [a], list(tails), "f30_sqr tail")


# ------------------------------------------------------------------------------- curve.hpp, jac<f30>
def jac_dbl_w(X, W, Z):
    a = M.sqr(X)
    b = M.sqr(W)
    d = M.mul(X, b)
    e = M.norm(M.mul3(a))
    z3 = M.mul(W, Z)
    x3 = sqr_tail(e, (-2, d))
    t = M.norm(M.sub(x3, d), 1)
    w3 = M.neg(M.mul_addsqr(e, t, b))
    return x3, w3, z3


def jac_tpl_affine_w(x, w):
    xx = M.sqr(x)
    yy = M.sqr(w)
    t = M.sqr(yy)
    m = M.norm(M.mul3(xx))
    mm = M.sqr(m)
    s = M.norm(M.mul3(M.mul(x, yy)))
    e = M.norm(M.sub(s, mm))
    ee = M.sqr(e)
    s = sqr_tail(M.norm(M.add(m, e)), (-1, mm), (-1, ee))
    u = M.norm(M.sub(s, t))
    x3 = M.norm(M.mul_sum2(x, ee, yy, M.neg(u)), 2)
    t = M.norm(M.sub(t, u))
    s = M.mul_sum2(u, t, e, M.neg(ee))
    w3 = M.norm(M.mul(w, s), 3)
    z3 = M.norm(e, 1)
    return x3, w3, z3


def jac_madd_w(X, W, Z, x2, w2, decide=True):
    """decide=False: a bounds-only run of the general branch"""
    z1z1 = M.sqr(Z)
    h = mul_tail(x2, z1z1, (-1, X))
    r = mul_tail(M.mul(w2, Z), z1z1, (-1, W))
    z1zero, hz, rz = M.is_zero(Z), M.is_zero(h), M.is_zero(r)
    if decide and z1zero:
        return x2, w2, M.one()
    if decide and hz and rz:
        return jac_dbl_w(X, W, Z)
    hh = M.sqr(h)
    z3 = M.mul(M.dbl(Z), h)
    i4 = M.norm(hh, 2)
    j = M.mul(h, i4)
    v = M.mul(X, i4)
    x3 = sqr_tail(r, (-1, j), (-2, v))
    vx = M.norm(M.sub(v, x3))
    w3 = M.mul_sum2(M.norm(r, 1), vx, M.norm(W, 1), M.neg(j))
    return x3, w3, z3


def mul_abs_u_affine(x, w, trace=None):
    X, W, Z = jac_tpl_affine_w(x, w)
    for b in range(M.ABS_U.bit_length() - 3, -1, -1):
        X, W, Z = jac_dbl_w(X, W, Z)
        if (M.ABS_U >> b) & 1:
            X, W, Z = jac_madd_w(X, W, Z, x, w)
        if trace is not None:
            trace.append((X, W, Z))
    return X, W, Z


def in_subgroup_fast_g1(x, w):
    q1 = mul_abs_u_affine(x, w)
    X, W, Z = mul_abs_u_affine(q1[0], q1[1])
    Z = M.mul(Z, q1[2])
    return M.jac_eq_affine(X, W, Z, M.mul(x, M.of_int(val(M.HDR["BETA30"]))), M.neg(w))
