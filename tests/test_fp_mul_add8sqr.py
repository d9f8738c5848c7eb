"""csrc/fp381.hpp fp_mul_add8sqr — (a b + 8 c^2) R^-1 mod p in one column scan, the c^2 half as a
squaring (cross products c_j (16 c_k) once, squares c_j (8 c_j)) — modelled step by step on Python
integers with every 64-bit accumulator checked, against plain modular arithmetic, at the operand
bounds the G1 doubling feeds it (curve.hpp jac_dbl: a = E normalized, b = F - 3D + KB_8_30 with limbs
below 2^30 + 2^28, c = B normalized). CPU only; the column bounds for the whole ladder are proven in
tests/test_field_bounds.py (field_bounds_model.mul_add8sqr)."""
import random

import pytest

from fp28_model import BLS, mul_addsqr

# the column scan is stated once, in tests/fp28_model.py (all six multiply forms, both fields)
P, N, LB, MASK, R, val = BLS.p, BLS.NL, BLS.LB, BLS.MASK, BLS.R, BLS.val


def mul_add8sqr(a, b, c, scale=8):
    return mul_addsqr(BLS, a, b, c, scale)


def rand_limbs(rng, limb_max, top_max):
    return [rng.randrange(limb_max + 1) for _ in range(N - 1)] + [rng.randrange(top_max + 1)]


@pytest.mark.parametrize("scale", [8, 1])
def test_mul_add8sqr_exact(scale):
    """scale 8: fp_mul_addsqr<8> (the Y-form doubling); scale 1: fp_mul_addsqr<1> (jac_dbl_w, whose
    b = 2 (X3 - D) has limbs below 2^31 + 2^29)."""
    rng = random.Random(8 + scale)
    top_n = (3 * P) >> (LB * (N - 1))          # normalized operands: values below ~3 p
    a_max, b_max = MASK, (1 << 30) + (1 << 28)  # E normalized; F - 3D + KB_8_30 lazy
    if scale == 1:
        b_max = 2 * b_max  # doubled
    cases = [([MASK] * (N - 1) + [top_n], [b_max] * (N - 1) + [top_n << 3], [MASK] * (N - 1) + [top_n])]
    for _ in range(400):
        cases.append((rand_limbs(rng, a_max, top_n), rand_limbs(rng, b_max, top_n << 3), rand_limbs(rng, MASK, top_n)))
    for a, b, c in cases:
        r = mul_add8sqr(a, b, c, scale)
        assert all(x <= MASK for x in r)
        assert (val(r) * R - (val(a) * val(b) + scale * val(c) ** 2)) % P == 0
