"""csrc/pairing_kernels.hip restated over Python integers, call for call: the same cells, the same
sequence of cell operations in the Miller loop's doubling and addition steps, the same coefficient
loops of x_mul / x_mul_line / x_frob, the same inversion and the same final-exponentiation chain.
tests/test_pairing_model.py checks it against the pairing's definition (tests/pairing_model.py), so a
wrong formula in the kernel's design shows on the CPU; tests/test_gpu_pairing.py then checks the kernel
itself against the definition.

A cell holds one Fq2 element as a pair of integers; the Frobenius table is the generated one
(tools/gen_pairing_constants.py), read here as integers.
"""
import os
import sys

import pairing_model as M

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import gen_pairing_constants as GEN  # noqa: E402

P, X_ABS = M.P, M.X_ABS
X_BITS = X_ABS.bit_length()
FROB = GEN.frobenius_table()
INV2 = pow(2, P - 2, P)

# the Miller kernel's cells
F, G, LINE, TX, TY, TZ, QX, QY, PXY = 0, 6, 12, 15, 16, 17, 18, 19, 20
S0, S1, S2, S3, S4, S5, S6, S7 = range(21, 29)
# the final exponentiation's
A, B, C, D, E, T, SCR = 0, 6, 12, 18, 24, 30, 36


class Cells(dict):
    """cell index -> Fq2"""

    def mul(m, d, a, b): m[d] = M.f2_mul(m[a], m[b])
    def sqr(m, d, a): m[d] = M.f2_mul(m[a], m[a])
    def add(m, d, a, b): m[d] = M.f2_add(m[a], m[b])
    def sub(m, d, a, b): m[d] = M.f2_sub(m[a], m[b])
    def neg(m, d, a): m[d] = M.f2_neg(m[a])
    def mul_xi(m, d, a): m[d] = M.f2_mul_xi(m[a])
    def half(m, d, a): m[d] = (m[a][0] * INV2 % P, m[a][1] * INV2 % P)
    def mul_fq(m, d, a, s, which): m[d] = (m[a][0] * m[s][which] % P, m[a][1] * m[s][which] % P)
    def inv(m, d, a): m[d] = M.f2_inv(m[a])

    def copy(m, d, src, a, n):
        for k in range(n):
            m[d + k] = src[a + k]

    def set_one(m, d, n):
        for k in range(n):
            m[d + k] = (1, 0) if k == 0 else (0, 0)


def xcell(n, base, e):
    return base + (e & 1) * 3 + (e >> 1) if n == 6 else base + e


def x_mul(md, d, ma, a, mb, b, n, square):
    out = {}
    for k in range(n):
        lo, hi = (0, 0), (0, 0)
        for i in range(n):
            wrap = i > k
            j = k - i + n if wrap else k - i
            if square and i > j:
                continue
            x = ma[xcell(n, a, i)]
            if square and i == j:
                t = M.f2_mul(x, x)
            else:
                t = M.f2_mul(x, mb[xcell(n, b, j)])
                if square:
                    t = M.f2_add(t, t)
            if wrap:
                hi = M.f2_add(hi, t)
            else:
                lo = M.f2_add(lo, t)
        out[xcell(n, d, k)] = M.f2_add(lo, M.f2_mul_xi(hi))
    # the kernel stores coefficient k before it reads the operands of k + 1: d overlaps no operand
    assert md is not ma or not set(out) & {xcell(n, a, i) for i in range(n)}
    assert md is not mb or not set(out) & {xcell(n, b, i) for i in range(n)}
    md.update(out)


def x_mul_line(m, d, a, l):
    assert d != a
    out = {}
    for k in range(6):
        lo, hi = (0, 0), (0, 0)
        for t in range(3):
            e = t + 1 if t else 0
            wrap = e > k
            i = k - e + 6 if wrap else k - e
            x = M.f2_mul(m[xcell(6, a, i)], m[l + t])
            if wrap:
                hi = M.f2_add(hi, x)
            else:
                lo = M.f2_add(lo, x)
        out[xcell(6, d, k)] = M.f2_add(lo, M.f2_mul_xi(hi))
    m.update(out)


def x_frob(m, d, a, k):
    for e in range(6):
        x = m[xcell(6, a, e)]
        if k & 1:
            x = M.f2_conj(x)
        m[xcell(6, d, e)] = M.f2_mul(x, FROB[k - 1][e])


def x_conj(m, d, a):
    if d != a:
        m.copy(d, m, a, 3)
    for k in range(3, 6):
        m.neg(d + k, a + k)


def x6_inv(m, d, a, s):
    m.sqr(s + 0, a + 0)
    m.mul(s + 3, a + 1, a + 2)
    m.mul_xi(s + 3, s + 3)
    m.sub(s + 0, s + 0, s + 3)
    m.sqr(s + 1, a + 2)
    m.mul_xi(s + 1, s + 1)
    m.mul(s + 3, a + 0, a + 1)
    m.sub(s + 1, s + 1, s + 3)
    m.sqr(s + 2, a + 1)
    m.mul(s + 3, a + 0, a + 2)
    m.sub(s + 2, s + 2, s + 3)
    m.mul(s + 3, a + 2, s + 1)
    m.mul(s + 4, a + 1, s + 2)
    m.add(s + 3, s + 3, s + 4)
    m.mul_xi(s + 3, s + 3)
    m.mul(s + 4, a + 0, s + 0)
    m.add(s + 3, s + 3, s + 4)
    m.inv(s + 3, s + 3)
    for k in range(3):
        m.mul(d + k, s + k, s + 3)


def x12_inv(m, d, a, s):
    x_mul(m, s + 0, m, a, m, a, 3, True)
    x_mul(m, s + 3, m, a + 3, m, a + 3, 3, True)
    m.mul_xi(s + 6, s + 5)
    m.sub(s + 0, s + 0, s + 6)
    m.sub(s + 1, s + 1, s + 3)
    m.sub(s + 2, s + 2, s + 4)
    x6_inv(m, s + 9, s + 0, s + 12)
    x_mul(m, d, m, a, m, s + 9, 3, False)
    x_mul(m, d + 3, m, a + 3, m, s + 9, 3, False)
    for k in range(3, 6):
        m.neg(d + k, d + k)


def miller_double(m):
    m.mul(S0, TX, TY)
    m.half(S0, S0)
    m.sqr(S1, TY)
    m.sqr(S2, TZ)
    m.add(S3, S2, S2)
    m.add(S3, S3, S2)
    m.add(S3, S3, S3)
    m.add(S3, S3, S3)
    m.mul_xi(S3, S3)
    m.add(S4, S3, S3)
    m.add(S4, S4, S3)
    m.add(S5, S1, S4)
    m.half(S5, S5)
    m.add(S6, TY, TZ)
    m.sqr(S6, S6)
    m.sub(S6, S6, S1)
    m.sub(S6, S6, S2)
    m.sub(LINE, S3, S1)
    m.sqr(S7, TX)
    m.sqr(S3, S3)
    m.sub(S4, S1, S4)
    m.mul(TX, S0, S4)
    m.sqr(S5, S5)
    m.add(S4, S3, S3)
    m.add(S4, S4, S3)
    m.sub(TY, S5, S4)
    m.mul(TZ, S1, S6)
    m.add(S4, S7, S7)
    m.add(S4, S4, S7)
    m.mul_fq(LINE + 1, S4, PXY, 0)
    m.neg(S6, S6)
    m.mul_fq(LINE + 2, S6, PXY, 1)


def miller_add(m):
    m.mul(S0, QY, TZ)
    m.sub(S0, TY, S0)
    m.mul(S1, QX, TZ)
    m.sub(S1, TX, S1)
    m.sqr(S2, S0)
    m.sqr(S3, S1)
    m.mul(S4, S1, S3)
    m.mul(S2, TZ, S2)
    m.mul(S3, TX, S3)
    m.add(S5, S4, S2)
    m.sub(S5, S5, S3)
    m.sub(S5, S5, S3)
    m.mul(TX, S1, S5)
    m.sub(S3, S3, S5)
    m.mul(S3, S0, S3)
    m.mul(S6, S4, TY)
    m.sub(TY, S3, S6)
    m.mul(TZ, TZ, S4)
    m.mul(S2, S0, QX)
    m.mul(S3, S1, QY)
    m.sub(LINE, S2, S3)
    m.neg(S0, S0)
    m.mul_fq(LINE + 1, S0, PXY, 0)
    m.mul_fq(LINE + 2, S1, PXY, 1)


def k_pair_miller(p, q):
    """one lane: p = (x, y) or None, q = ((x0, x1), (y0, y1)) or None -> the lane's cells"""
    m = Cells()
    m.set_one(F, 6)
    if p is None or q is None:
        return m
    m[PXY] = (p[0], p[1])
    m[QX], m[QY], m[TX], m[TY] = q[0], q[1], q[0], q[1]
    m.set_one(TZ, 1)
    for b in range(X_BITS - 2, -1, -1):
        x_mul(m, G, m, F, m, F, 6, True)
        miller_double(m)
        x_mul_line(m, F, G, LINE)
        if (X_ABS >> b) & 1:
            miller_add(m)
            x_mul_line(m, G, F, LINE)
            m.copy(F, m, G, 6)
    return m


def k_pair_tree(lanes):
    """the stride form of the block's tree: after it lane 0 holds the product"""
    count, s = len(lanes), 1
    while s < count:
        for g in range(0, count, 2 * s):
            if g + s < count:
                x_mul(lanes[g], G, lanes[g], F, lanes[g + s], F, 6, False)
                lanes[g].copy(F, lanes[g], G, 6)
        s *= 2


def x12_mul(m, d, a, b): x_mul(m, d, m, a, m, b, 6, False)
def x12_sqr(m, d, a): x_mul(m, d, m, a, m, a, 6, True)


def x12_pow_x(m, d, a):
    cur, oth = d, T
    m.copy(cur, m, a, 6)
    for b in range(X_BITS - 2, -1, -1):
        x12_sqr(m, oth, cur)
        cur, oth = oth, cur
        if (X_ABS >> b) & 1:
            x12_mul(m, oth, cur, a)
            cur, oth = oth, cur
    if cur != d:
        m.copy(d, m, cur, 6)


def k_pair_final(lane0):
    """lane0: the cells holding the product of the Miller values (None: k = 0) -> the Fq12 result"""
    m = Cells()
    if lane0 is not None:
        m.copy(A, lane0, F, 6)
    else:
        m.set_one(A, 6)
    x_conj(m, A, A)
    x_conj(m, B, A)
    x12_inv(m, C, A, SCR)
    x12_mul(m, D, B, C)
    x_frob(m, B, D, 2)
    x12_mul(m, A, B, D)
    x12_pow_x(m, B, A)
    x_conj(m, B, B)
    x_conj(m, C, A)
    x12_mul(m, D, B, C)
    x12_pow_x(m, B, D)
    x_conj(m, B, B)
    x_conj(m, C, D)
    x12_mul(m, E, B, C)
    x12_pow_x(m, B, E)
    x_conj(m, B, B)
    x_frob(m, C, E, 1)
    x12_mul(m, D, B, C)
    x12_pow_x(m, B, D)
    x12_pow_x(m, C, B)
    x_frob(m, B, D, 2)
    x12_mul(m, E, C, B)
    x_conj(m, B, D)
    x12_mul(m, C, E, B)
    x12_sqr(m, B, A)
    x12_mul(m, D, B, A)
    x12_mul(m, E, C, D)
    return cells_to_f12(m, E)


def cells_to_f12(m, base):
    """six cells in ark's order -> pairing_model's Fq12"""
    return (tuple(m[base + k] for k in range(3)), tuple(m[base + 3 + k] for k in range(3)))


def pairing_product(pairs):
    lanes = [k_pair_miller(p, q) for p, q in pairs]
    k_pair_tree(lanes)
    return k_pair_final(lanes[0] if lanes else None)
