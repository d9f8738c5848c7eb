"""csrc/fp381.hpp fp_mul_add8sqr — (a b + 8 c^2) R^-1 mod p in one column scan, the c^2 half as a
squaring (cross products c_j (16 c_k) once, squares c_j (8 c_j)) — modelled step by step on Python
integers with every 64-bit accumulator checked, against plain modular arithmetic, at the operand
bounds the G1 doubling feeds it (curve.hpp jac_dbl: a = E normalized, b = F - 3D + KB_8_30 with limbs
below 2^30 + 2^28, c = B normalized). CPU only; the column bounds for the whole ladder are proven in
tests/test_field_bounds.py (field_bounds_model.mul_add8sqr)."""
import random

import pytest

from fp28_model import BLS
from fp28_model import mul_add8sqr as scan_add8sqr

# the column scan is stated once, in tests/fp28_model.py (all five multiply forms, both fields)
P, N, LB, MASK, R, val = BLS.p, BLS.NL, BLS.LB, BLS.MASK, BLS.R, BLS.val


def mul_add8sqr(a, b, c):
    return scan_add8sqr(BLS, a, b, c)


def rand_limbs(rng, limb_max, top_max):
    return [rng.randrange(limb_max + 1) for _ in range(N - 1)] + [rng.randrange(top_max + 1)]


@pytest.mark.parametrize("scale", [8])
def test_mul_add8sqr_exact(scale):
    """scale 8, the only one: the Y-form doubling's -Y3 = E (X3 - D) + 8 B^2"""
    rng = random.Random(8 + scale)
    top_n = (3 * P) >> (LB * (N - 1))          # normalized operands: values below ~3 p
    a_max, b_max = MASK, (1 << 30) + (1 << 28)  # E normalized; F - 3D + KB_8_30 lazy
    cases = [([MASK] * (N - 1) + [top_n], [b_max] * (N - 1) + [top_n << 3], [MASK] * (N - 1) + [top_n])]
    for _ in range(400):
        cases.append((rand_limbs(rng, a_max, top_n), rand_limbs(rng, b_max, top_n << 3), rand_limbs(rng, MASK, top_n)))
    for a, b, c in cases:
        r = mul_add8sqr(a, b, c)
        assert all(x <= MASK for x in r)
        assert (val(r) * R - (val(a) * val(b) + scale * val(c) ** 2)) % P == 0
