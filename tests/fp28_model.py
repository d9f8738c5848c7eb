"""Exact value-level model of the 14 x 28 / 9 x 29 limb core in csrc/fp381.hpp, on Python integers, for
both fields (p, NL, LB from field_bounds_model.FIELDS; the constants read from the .hpp files, -p^-1
derived and compared with the header's).

  * scan(): the column scan of the five multiply forms (fp_mul, fp_sqr, fp_mul_sum2, fp_mul_sum3,
    fp_mul_add8sqr) with the device's accumulators — acc, acc2, acc3 and accp — each checked
    against uint64 at every step, every doubled or scaled limb against uint32, and the carry out of
    the last column against zero (the result would not fit NL limbs). The interval proof of
    tests/field_bounds_model.py bounds the column SUMS; this follows the chains the device keeps.
    bits=63 / doubling=False are the deliberately wrong variants the tests use to show that their
    operands would expose a 63-bit accumulator or a squaring without its doubling.
  * plain restatements of the limb-wise forms, reductions, comparisons, zero tests and word
    conversions, step by step as the device does them, each raising where a 32-bit register or a
    signed borrow chain would leave its range; the 13 x 30 conversions and f30_is_zero are those of
    tests/f30_ladder_model.py.
tests/test_gpu_fp28_core.py runs every function on the GPU against these, limb for limb."""
import os
import re

import f30_ladder_model as L
import field_bounds_model as M

CSRC = os.path.dirname(M.CONSTS)
U32 = 0xFFFFFFFF


def u64(x, what):
    if not 0 <= x < 1 << 64:
        raise OverflowError(f"{what}: {x:#x} leaves uint64")
    return x


def u32(x, what):
    if not 0 <= x < 1 << 32:
        raise OverflowError(f"{what}: {x:#x} leaves uint32")
    return x


def i32(x, what):
    if not -(1 << 31) <= x < 1 << 31:
        raise OverflowError(f"{what}: {x:#x} leaves int32")
    return x


class Field:
    def __init__(self, name):
        self.name = name
        self.p, self.NL, self.LB, hdr = M.FIELDS[name]
        self.MASK = (1 << self.LB) - 1
        self.R = 1 << (self.LB * self.NL)
        self.PL = self.limbs(self.p)
        self.PINV = (-pow(self.p, -1, 1 << self.LB)) % (1 << self.LB)
        path = os.path.join(CSRC, hdr)
        text = open(path).read().split("\n};")[0]  # the traits struct
        self.C = M.load_consts(path)
        self.NW = int(re.search(r"int NW = (\d+);", text).group(1))
        self.INV_RHO = float(re.search(r"INV_RHO = ([0-9.e+-]+);", text).group(1))
        # a borrowed constant's comment: "<m> p, limbs >= 2^<x> - 2^<y>, dominates values < <v> p"
        self.KB = {}
        for n, m, x, y, v in re.findall(
                r"uint32_t (KB_\w+)\[\d+\] = \{[^}]*\};\s*// (\d+) p, limbs >= 2\^(\d+) - 2\^(\d+), dominates values < ([0-9.]+) p",
                text):
            self.KB[n] = (int(m), (1 << int(x)) - (1 << int(y)), float(v))
        # the header agrees with the derivations
        assert self.C["P"] == self.PL and self.C["P_X1"] == self.PL
        assert int(re.search(r"PINV = (0x[0-9a-f]+)u;", text).group(1), 16) == self.PINV
        assert int(re.search(r"int NL = (\d+);", text).group(1)) == self.NL
        assert int(re.search(r"int LB = (\d+);", text).group(1)) == self.LB
        assert self.val(self.C["R2"]) == self.R * self.R % self.p and self.val(self.C["ONE"]) == self.R % self.p
        for k in (1, 2, 4, 8, 16, 32, 64, 128):
            assert self.C[f"P_X{k}"] == self.limbs(k * self.p)
        for n, (m, _, _) in self.KB.items():
            assert self.val(self.C[n]) == m * self.p, n
        self.kmax = min(256, self.R // self.p)  # fp_canon / fp_is_zero: value < kmax p

    def val(self, limbs):
        return sum(x << (self.LB * k) for k, x in enumerate(limbs))

    def limbs(self, x):
        """normalized limbs of x >= 0; the top limb takes the rest"""
        return [(x >> (self.LB * k)) & self.MASK for k in range(self.NL - 1)] + [x >> (self.LB * (self.NL - 1))]


BLS = Field("bls12_381")
BN254 = Field("bn254")
FIELD = {"bls12_381": BLS, "bn254": BN254}


# ------------------------------------------------------------------------------- multiply forms
def scan(F, prods, sq=None, scale=1, sq_in_acc=False, bits=64, doubling=True, stats=None):
    """(sum of a b over prods [+ scale sq^2]) R^-1 mod p as the device scans it: the first product's
    chain runs on acc (on top of the incoming carry), the second and third on acc2 and acc3, m p on
    accp; a square is cross products once, sq_j (2 scale sq_k), plus the diagonal sq_j (scale sq_j), on
    acc2 (fp_mul_add8sqr) or on acc (fp_sqr: sq_in_acc). bits = 64 raises OverflowError when an
    accumulator leaves uint64; a smaller bits WRAPS instead (the wrong device a test must tell apart).
    stats["peak"]: the largest accumulator value seen."""
    N, LB, MASK, PL = F.NL, F.LB, F.MASK, F.PL
    assert len(prods) <= 3 and (sq is None or len(prods) <= 1)
    peak = 0

    def acc_add(x, y, what):
        nonlocal peak
        s = x + y
        peak = max(peak, s)
        return u64(s, what) if bits == 64 else s & ((1 << bits) - 1)

    if sq is not None:
        s1 = [u32(x * scale, "scaled limb") for x in sq]
        s2 = [u32(2 * x, "doubled limb") for x in s1] if doubling else s1
    m, r, acc = [0] * N, [0] * N, 0
    for i in range(2 * N):
        j0 = 0 if i < N else i - (N - 1)
        j1 = i - 1 if i < N else N - 1
        accs = [0, 0, 0]
        accs[0] = acc
        accp = 0
        for j in range(j0, j1 + 1):
            for t, (a, b) in enumerate(prods):
                accs[t] = acc_add(accs[t], a[j] * b[i - j], ("acc", "acc2", "acc3")[t])
            accp = acc_add(accp, m[j] * PL[i - j], "accp")
        if sq is not None:
            t = 0 if sq_in_acc else 1
            for j in range(j0, N):
                if 2 * j < i and i - j < N:
                    accs[t] = acc_add(accs[t], sq[j] * s2[i - j], "square chain")
            if i % 2 == 0 and i // 2 < N:
                accs[t] = acc_add(accs[t], sq[i // 2] * s1[i // 2], "square chain")
        if i < N:
            for t, (a, b) in enumerate(prods):
                accs[t] = acc_add(accs[t], a[i] * b[0], ("acc", "acc2", "acc3")[t])
        rest = 0
        for x in accs[1:] + [accp]:
            rest = acc_add(rest, x, "acc2 + acc3 + accp")
        acc = acc_add(accs[0], rest, "acc")
        if i < N:
            m[i] = ((acc & U32) * F.PINV) & MASK
            acc = acc_add(acc, m[i] * PL[0], "acc")
            assert bits != 64 or acc & MASK == 0
        else:
            r[i - N] = acc & MASK
        acc >>= LB
    if bits == 64 and acc:
        raise OverflowError(f"the carry out of the last column is {acc:#x}: the result does not fit {N} limbs")
    if stats is not None:
        stats["peak"] = max(stats.get("peak", 0), peak)
    return r


def mul(F, a, b, **kw):
    return scan(F, [(a, b)], **kw)


def sqr(F, a, **kw):
    return scan(F, [], sq=a, sq_in_acc=True, **kw)


def mul_sum2(F, a, b, c, d, **kw):
    return scan(F, [(a, b), (c, d)], **kw)


def mul_sum3(F, a, b, c, d, e, f, **kw):
    return scan(F, [(a, b), (c, d), (e, f)], **kw)


def mul_add8sqr(F, a, b, c, **kw):
    return scan(F, [(a, b)], sq=c, scale=8, **kw)


# ------------------------------------------------------------------------------- limb-wise forms
def add_nr(F, a, b):
    return [u32(x + y, "add") for x, y in zip(a, b)]


def shl_nr(F, a, s):
    return [u32(x << s, "shl") for x in a]


def subk(F, kname, a, b):
    """fp_subk_nr<K>: (a + K) - b limb by limb"""
    K = F.C[kname]
    return [u32(u32(x + k, f"{kname} add") - y, f"{kname} sub") for x, k, y in zip(a, K, b)]


def negk(F, kname, b):
    return [u32(k - y, f"{kname} neg") for k, y in zip(F.C[kname], b)]


def norm(F, a):
    r, c = [], 0
    for i in range(F.NL - 1):
        t = u32(a[i] + c, "norm")
        r.append(t & F.MASK)
        c = t >> F.LB
    return r + [u32(a[F.NL - 1] + c, "norm top")]


def add(F, a, b):
    return norm(F, add_nr(F, a, b))


def half(F, a):
    """fp_half: a normalized below the top limb; + p if odd, one right shift across the limbs"""
    assert all(x <= F.MASK for x in a[:-1]), "fp_half: input not normalized"
    odd = a[0] & 1
    t, c = [], 0
    for i in range(F.NL - 1):
        s = u32(a[i] + (F.PL[i] if odd else 0) + c, "half")
        t.append(s & F.MASK)
        c = s >> F.LB
    t.append(u32(a[-1] + (F.PL[-1] if odd else 0) + c, "half top"))
    return [(t[i] >> 1) | ((t[i + 1] & 1) << (F.LB - 1)) for i in range(F.NL - 1)] + [t[-1] >> 1]


def sub_borrow(F, a, k):
    """fp_sub_const_borrow: signed chain a - k; (borrow, difference limbs). Both below 2^31 per limb."""
    d, br = [], 0
    for x, y in zip(a, k):
        assert x < 1 << 31 and y < 1 << 31, "signed borrow chain on a limb >= 2^31"
        t = i32(x - y + br, "borrow chain")
        d.append(t & F.MASK)
        br = t >> F.LB
        assert br in (0, -1), "the borrow chain needs normalized operands"
    return br != 0, d


def reduce_once(F, a):
    b, d = sub_borrow(F, a, F.PL)
    return list(a) if b else d


def reduce_canon(F, a):
    x = list(a)
    for k in (128, 64, 32, 16, 8, 4, 2, 1):
        b, d = sub_borrow(F, x, F.C[f"P_X{k}"])
        x = x if b else d
    return x


def canon(F, a):
    return reduce_canon(F, norm(F, a))


def is_zero(F, a):
    """fp_is_zero, per lane (the wave-uniform early exit changes no lane's answer)"""
    kc = (((a[0] & F.MASK) * ((-F.PINV) & U32)) & U32) & F.MASK
    if kc >= 256:
        return False
    n = norm(F, a)
    k = int(float(u32(n[-1] + 1, "top + 1")) * F.INV_RHO)
    assert 0 <= k < 1 << 32
    c, diff = 0, 0
    for i in range(F.NL - 1):
        c = u64(c + k * F.PL[i], "is_zero")
        diff |= (c & F.MASK) ^ n[i]
        c >>= F.LB
    c = u64(c + k * F.PL[-1], "is_zero")
    diff |= (c & U32) ^ n[-1]
    return diff == 0


def filter_candidate(F, a):
    """the k_c of fp_is_zero's low-limb filter: the lane takes the full test iff it is below 256"""
    return (((a[0] & F.MASK) * ((-F.PINV) & U32)) & U32) & F.MASK


def eq(F, a, b):
    return is_zero(F, subk(F, "KB_EQ", a, b))


def lt_canon(F, a, b):
    return sub_borrow(F, a, b)[0]


def neg_canon(F, c):
    if not any(c):
        return [0] * F.NL
    b, d = sub_borrow(F, F.PL, c)
    return d


def cond_sub_2p(F, a):
    b, d = sub_borrow(F, a, F.C["P_X2"])
    return list(a) if b else d


def add_red(F, a, b):
    return cond_sub_2p(F, norm(F, add_nr(F, a, b)))


def sub_red(F, a, b):
    neg, d = sub_borrow(F, a, b)
    e, c = [], 0
    for i in range(F.NL):
        t = u32(d[i] + F.C["P_X2"][i] + c, "sub_red")
        e.append(t & F.MASK)
        c = t >> F.LB
    return e if neg else d


def f2_mul(F, a0, a1, b0, b1):
    nb1 = negk(F, "KB_4_28", b1)
    return mul_sum2(F, a0, b0, a1, nb1), mul_sum2(F, a0, b1, a1, b0)


def f2_sqr(F, a0, a1):
    s, d, t = add_nr(F, a0, a1), subk(F, "KB_4_28", a0, a1), shl_nr(F, a0, 1)
    return mul(F, s, d), mul(F, t, a1)


# ------------------------------------------------------------------------------- words, Montgomery form
def from_words(F, w):
    r = []
    for k in range(F.NL):
        bit = F.LB * k
        i, off = bit >> 5, bit & 31
        lo = w[i] >> off if i < F.NW else 0
        hi = (w[i + 1] << (32 - off)) & U32 if off > 32 - F.LB and i + 1 < F.NW else 0
        r.append((lo | hi) & F.MASK)
    return r


def to_words(F, c):
    w = []
    for j in range(F.NW):
        bit = 32 * j
        k, off = bit // F.LB, bit % F.LB
        v = c[k] >> off
        if k + 1 < F.NL:
            v |= (c[k + 1] << (F.LB - off)) & U32
        if 2 * F.LB - off < 32 and k + 2 < F.NL:
            v |= (c[k + 2] << (2 * F.LB - off)) & U32
        w.append(v & U32)
    return w


def to_mont(F, c):
    return mul(F, c, F.C["R2"])


def from_mont(F, a):
    return reduce_once(F, mul(F, a, [1] + [0] * (F.NL - 1)))


# ------------------------------------------------------------------------------- 14 x 28 <-> 13 x 30 (BLS12-381)
def f30_from_fp(a):
    return L.f30_from_fp(norm(BLS, a))


def fp_from_f30(z):
    return L.fp_from_f30(z)


def f30_from_mont(h, a):
    return L.from_mont(h, a).d


def fp_mont_from_f30(h, z):
    v = P_1001
    return L.mont_from_f30(h, L.V(z, L.B(max(abs(x) for x in z[:-1]), abs(z[-1]), v)))


def f30_is_zero(z, k=L.ZK):
    return L.is_zero(L.V(z, L.B(max(abs(x) for x in z[:-1]), abs(z[-1]), max(abs(L.val(z)), 1))), k)


P_1001 = BLS.p + BLS.p // 1000
