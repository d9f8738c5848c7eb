"""The BLS12-381 pairing over Python integers, from its definition: the reference of tests/test_gpu_pairing.py
and tests/test_gpu_kzg_check.py.

Kept independent of csrc/pairing_kernels.hip on purpose. The kernel runs the Miller loop on the twist in
homogeneous projective coordinates with sparse lines and finishes with a Frobenius / exponentiation-by-|x|
chain; this file maps Q to E(Fq12), runs the textbook affine Miller loop there with dense Fq12 arithmetic
(one Fq12 inversion per slope), and raises the conjugated Miller value to d (p^12 - 1) / r by plain
square-and-multiply. Nothing is imported from oracle/ for the pairing itself.

Tower (ark-bls12-381's): Fq2 = Fq[u] / (u^2 + 1), Fq6 = Fq2[v] / (v^3 - (u + 1)), Fq12 = Fq6[w] / (w^2 - v).
Fq2 elements are pairs of ints, Fq6 triples of Fq2, Fq12 pairs of Fq6. The twist E': y^2 = x^3 + 4 (u + 1)
is of M type: (x', y') -> (x' / w^2, y' / w^3) maps E'(Fq2) into E(Fq12).
"""
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X_ABS = 0xD201000000010000  # the loop parameter is x = -X_ABS
D = 3                       # KZGPOT_PAIRING_GT_POWER: the library's GT value is e(P, Q)^D
XI = (1, 1)

assert (P ** 12 - 1) % R == 0


# ------------------------------------------------------------------------------------------ Fq2
def f2_add(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
def f2_sub(a, b): return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
def f2_neg(a): return (-a[0] % P, -a[1] % P)
def f2_mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)
def f2_conj(a): return (a[0], -a[1] % P)
def f2_mul_xi(a): return ((a[0] - a[1]) % P, (a[0] + a[1]) % P)


def f2_inv(a):
    t = pow(a[0] * a[0] + a[1] * a[1], P - 2, P)
    return (a[0] * t % P, -a[1] * t % P)


def f2_pow(a, e):
    acc = (1, 0)
    for bit in bin(e)[2:]:
        acc = f2_mul(acc, acc)
        if bit == "1":
            acc = f2_mul(acc, a)
    return acc


F2_ZERO, F2_ONE = (0, 0), (1, 0)


# ------------------------------------------------------------------------------------------ Fq6
def f6_add(a, b): return tuple(f2_add(x, y) for x, y in zip(a, b))
def f6_sub(a, b): return tuple(f2_sub(x, y) for x, y in zip(a, b))
def f6_neg(a): return tuple(f2_neg(x) for x in a)
def f6_mul_v(a): return (f2_mul_xi(a[2]), a[0], a[1])


def f6_mul(a, b):
    """schoolbook, v^3 = xi"""
    t = [F2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            t[i + j] = f2_add(t[i + j], f2_mul(a[i], b[j]))
    return (f2_add(t[0], f2_mul_xi(t[3])), f2_add(t[1], f2_mul_xi(t[4])), t[2])


def f6_inv(a):
    c0 = f2_sub(f2_mul(a[0], a[0]), f2_mul_xi(f2_mul(a[1], a[2])))
    c1 = f2_sub(f2_mul_xi(f2_mul(a[2], a[2])), f2_mul(a[0], a[1]))
    c2 = f2_sub(f2_mul(a[1], a[1]), f2_mul(a[0], a[2]))
    t = f2_add(f2_mul(a[0], c0), f2_mul_xi(f2_add(f2_mul(a[2], c1), f2_mul(a[1], c2))))
    t = f2_inv(t)
    return (f2_mul(c0, t), f2_mul(c1, t), f2_mul(c2, t))


F6_ZERO, F6_ONE = (F2_ZERO,) * 3, (F2_ONE, F2_ZERO, F2_ZERO)


# ------------------------------------------------------------------------------------------ Fq12
F12_ONE = (F6_ONE, F6_ZERO)
F12_W = (F6_ZERO, F6_ONE)


def f12_add(a, b): return (f6_add(a[0], b[0]), f6_add(a[1], b[1]))
def f12_sub(a, b): return (f6_sub(a[0], b[0]), f6_sub(a[1], b[1]))
def f12_conj(a): return (a[0], f6_neg(a[1]))


def f12_mul(a, b):
    """schoolbook, w^2 = v"""
    return (f6_add(f6_mul(a[0], b[0]), f6_mul_v(f6_mul(a[1], b[1]))),
            f6_add(f6_mul(a[0], b[1]), f6_mul(a[1], b[0])))


def f12_inv(a):
    t = f6_inv(f6_sub(f6_mul(a[0], a[0]), f6_mul_v(f6_mul(a[1], a[1]))))
    return (f6_mul(a[0], t), f6_neg(f6_mul(a[1], t)))


def f12_pow(a, e):
    acc = F12_ONE
    for bit in bin(e)[2:]:
        acc = f12_mul(acc, acc)
        if bit == "1":
            acc = f12_mul(acc, a)
    return acc


def f12_from_fq(x): return (((x % P, 0), F2_ZERO, F2_ZERO), F6_ZERO)
def f12_from_fq2(x): return ((x, F2_ZERO, F2_ZERO), F6_ZERO)


def f12_frobenius(a, k):
    """a^(p^k), by definition"""
    return f12_pow(a, P ** k)


# ------------------------------------------------------------------------------------------ the pairing
_W2_INV = f12_inv(f12_mul(F12_W, F12_W))
_W3_INV = f12_inv(f12_mul(F12_W, f12_mul(F12_W, F12_W)))


def untwist(q):
    """(x', y') on E'(Fq2) -> (x' / w^2, y' / w^3) on E(Fq12)"""
    return (f12_mul(f12_from_fq2(q[0]), _W2_INV), f12_mul(f12_from_fq2(q[1]), _W3_INV))


def _line(t, lam, xp, yp):
    """the line through t with slope lam, at (xp, yp)"""
    return f12_sub(f12_sub(yp, t[1]), f12_mul(lam, f12_sub(xp, t[0])))


def _step(t, s, lam):
    """t + s on y^2 = x^3 + 4 for the slope lam of the line through both"""
    x3 = f12_sub(f12_sub(f12_mul(lam, lam), t[0]), s[0])
    return (x3, f12_sub(f12_mul(lam, f12_sub(t[0], x3)), t[1]))


def miller_loop(p, q):
    """f_{|x|, Q}(P) for affine P = (x, y) in E(Fq) and Q = (x', y') in E'(Fq2); None is the point at infinity"""
    if p is None or q is None:
        return F12_ONE
    xp, yp = f12_from_fq(p[0]), f12_from_fq(p[1])
    qq = untwist(q)
    three, two = f12_from_fq(3), f12_from_fq(2)
    t, f = qq, F12_ONE
    for bit in bin(X_ABS)[3:]:
        lam = f12_mul(f12_mul(three, f12_mul(t[0], t[0])), f12_inv(f12_mul(two, t[1])))
        f = f12_mul(f12_mul(f, f), _line(t, lam, xp, yp))
        t = _step(t, t, lam)
        if bit == "1":
            lam = f12_mul(f12_sub(t[1], qq[1]), f12_inv(f12_sub(t[0], qq[0])))
            f = f12_mul(f, _line(t, lam, xp, yp))
            t = _step(t, qq, lam)
    return f


FINAL_EXPONENT = D * ((P ** 12 - 1) // R)


def final_exponentiation(f):
    """x < 0: the Miller value of the loop over |x| is conjugated, then raised to d (p^12 - 1) / r"""
    return f12_pow(f12_conj(f), FINAL_EXPONENT)


def pairing(p, q):
    """e(P, Q)^D"""
    return final_exponentiation(miller_loop(p, q))


def pairing_product(pairs):
    acc = F12_ONE
    for p, q in pairs:
        acc = f12_mul(acc, miller_loop(p, q))
    return final_exponentiation(acc)


# ------------------------------------------------------------------------------------------ bytes
def f12_coeffs(a):
    """the twelve Fq coefficients in ark's serialization order: c0.c0.c0, c0.c0.c1, c0.c1.c0, .., c1.c2.c1"""
    return [c for half in a for e in half for c in e]


def f12_to_bytes(a) -> bytes:
    return b"".join(c.to_bytes(48, "little") for c in f12_coeffs(a))


def f12_from_bytes(b: bytes):
    assert len(b) == 576
    c = [int.from_bytes(b[48 * i: 48 * i + 48], "little") for i in range(12)]
    assert all(x < P for x in c)
    e = [(c[2 * i], c[2 * i + 1]) for i in range(6)]
    return (tuple(e[:3]), tuple(e[3:]))


GT_ONE_BYTES = f12_to_bytes(F12_ONE)
