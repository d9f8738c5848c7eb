"""The constants of the pairing's final exponentiation (csrc/pairing_kernels.hip), derived from p with
Python integers; tools/gen_constants.py appends them to csrc/bls12_381_consts.hpp.

Frobenius on Fq12 = Fq2[w] / (w^6 - xi), xi = u + 1: an element is sum_e b_e w^e with b_e in Fq2, and
    (b_e w^e)^(p^k) = conj^k(b_e) w^e gamma_k^e,    gamma_k = w^(p^k - 1) = xi^((p^k - 1) / 6) in Fq2,
so the table holds gamma_k^e for k = 1, 2 and e = 0 .. 5 (tests/test_pairing_model.py recomputes it).
"""
from __future__ import annotations

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X = -0xD201000000010000
XI = (1, 1)
GT_POWER = 3  # the hard-part chain computes f^(3 (p^4 - p^2 + 1) / r)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_pow(a, e):
    acc = (1, 0)
    for bit in bin(e)[2:]:
        acc = f2_mul(acc, acc)
        if bit == "1":
            acc = f2_mul(acc, a)
    return acc


def frobenius_table():
    """[k - 1][e] = gamma_k^e as an Fq2 pair of integers"""
    table = []
    for k in (1, 2):
        assert (P ** k - 1) % 6 == 0
        gamma = f2_pow(XI, (P ** k - 1) // 6)
        row, acc = [], (1, 0)
        for _ in range(6):
            row.append(acc)
            acc = f2_mul(acc, gamma)
        assert acc == f2_pow(XI, P ** k - 1)  # gamma^6 = xi^(p^k - 1)
        table.append(row)
    assert all(c[1] == 0 for c in table[1])  # k = 2: the factors lie in Fq
    return table


def check_hard_part():
    """the chain's exponent: (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3 = 3 (p^4 - p^2 + 1) / r"""
    assert (P ** 4 - P ** 2 + 1) % R == 0
    assert (X - 1) ** 2 * (X + P) * (X * X + P * P - 1) + 3 == GT_POWER * ((P ** 4 - P ** 2 + 1) // R)


def header_lines(limbs, mont):
    """limbs: int -> the field core's limb list; mont: int -> its Montgomery form"""
    check_hard_part()
    rows = []
    for row in frobenius_table():
        rows.append("{" + ", ".join(
            "{" + ", ".join("{" + ", ".join(f"0x{v:08x}u" for v in limbs(mont(c))) + "}" for c in e) + "}"
            for e in row) + "}")
    return [
        "// the pairing's Frobenius maps (csrc/pairing_kernels.hip; tools/gen_pairing_constants.py):",
        "// FP12_FROB[k - 1][e][c] = component c of xi^(e (p^k - 1) / 6) in Fq2, Montgomery form, k = 1, 2, e = 0 .. 5",
        "static constexpr uint32_t FP12_FROB[2][6][2][14] = {" + ", ".join(rows) + "};",
    ]


if __name__ == "__main__":
    check_hard_part()
    for k, row in enumerate(frobenius_table(), 1):
        for e, c in enumerate(row):
            print(f"gamma_{k}^{e} = ({c[0]:#x}, {c[1]:#x})")
