"""The pairing model (tests/pairing_model.py) is a pairing, the generated Frobenius constants are what
they claim to be, the kernel's formulas (tests/pairing_kernel_model.py) compute the model's value, and
the batch_check equation holds in the model alone. CPU only; generators come from the oracle."""
import os
import random
import re

import pytest

import kzgpot_oracle as O
import pairing_kernel_model as K
import pairing_model as M

P, R = O.P, O.R_ORDER
G1, G2 = O.G1_GEN, O.G2_GEN
HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kzg-setup-powersoftau_amd", "csrc",
                   "bls12_381_consts.hpp")


@pytest.fixture(scope="module")
def e_gen():
    return M.pairing(G1, G2)


def test_model_constants_are_the_oracles():
    assert (M.P, M.R, -M.X_ABS) == (O.P, O.R_ORDER, O.U_PARAM)
    assert O.B2 == (4 * M.XI[0], 4 * M.XI[1])


def test_nondegenerate_and_of_order_r(e_gen):
    assert e_gen != M.F12_ONE
    assert M.f12_pow(e_gen, R) == M.F12_ONE


def test_bilinear(e_gen):
    rng = random.Random(1)
    for _ in range(2):
        a, b = rng.randrange(1, 1 << 16), rng.randrange(1, 1 << 16)
        assert M.pairing(O.g1_mul(G1, a), O.g2_mul(G2, b)) == M.f12_pow(e_gen, a * b)


def test_inverse_pair_and_infinity(e_gen):
    neg = (G1[0], -G1[1] % P)
    assert M.f12_mul(e_gen, M.pairing(neg, G2)) == M.F12_ONE
    assert M.pairing_product([(G1, G2), (neg, G2)]) == M.F12_ONE
    assert M.pairing(None, G2) == M.pairing(G1, None) == M.F12_ONE
    assert M.pairing_product([]) == M.F12_ONE


def test_bytes_round_trip(e_gen):
    b = M.f12_to_bytes(e_gen)
    assert len(b) == 576 and M.f12_from_bytes(b) == e_gen
    assert M.GT_ONE_BYTES == (1).to_bytes(48, "little") + bytes(528)


# ------------------------------------------------------------------------------------- the generated constants
def header_frobenius():
    """FP12_FROB as integers: [k - 1][e] = (c0, c1), out of Montgomery form"""
    text = open(HDR).read()
    m = re.search(r"FP12_FROB\[2\]\[6\]\[2\]\[14\] = (\{.*?\});", text)
    limbs = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{8})u", m.group(1))]
    assert len(limbs) == 2 * 6 * 2 * 14
    rinv = pow(1 << 392, -1, P)
    vals = [sum(v << (28 * i) for i, v in enumerate(limbs[14 * j: 14 * j + 14])) * rinv % P for j in range(24)]
    return [[(vals[12 * k + 2 * e], vals[12 * k + 2 * e + 1]) for e in range(6)] for k in range(2)]


def test_frobenius_constants_recomputed():
    table = header_frobenius()
    assert table == K.FROB
    for k in (1, 2):
        gamma = M.f2_pow(M.XI, (P ** k - 1) // 6)
        for e in range(6):
            assert table[k - 1][e] == M.f2_pow(gamma, e)


def test_frobenius_by_constants_is_the_power_map(e_gen):
    """x_frob's rule (conjugate each coefficient, multiply by gamma_k^e) against a^(p^k) by definition"""
    a = M.f12_mul(M.miller_loop(G1, G2), e_gen)  # a generic element, not in a subfield
    for k in (1, 2):
        m = K.Cells()
        m.copy(0, {i: c for i, c in enumerate(a[0] + a[1])}, 0, 6)
        K.x_frob(m, 6, 0, k)
        assert K.cells_to_f12(m, 6) == M.f12_frobenius(a, k)


def test_hard_part_exponent():
    x = -M.X_ABS
    assert (x - 1) ** 2 * (x + P) * (x * x + P * P - 1) + 3 == M.D * ((P ** 4 - P ** 2 + 1) // R)
    assert M.FINAL_EXPONENT == (P ** 6 - 1) * (P ** 2 + 1) * M.D * ((P ** 4 - P ** 2 + 1) // R)
    assert M.D % R != 0  # e^D = 1 iff e = 1 in the group of order r


# ------------------------------------------------------------------------------------- the kernel's formulas
def test_kernel_formulas_give_the_models_value(e_gen):
    assert K.pairing_product([(G1, G2)]) == e_gen
    rng = random.Random(2)
    p, q = O.g1_mul(G1, rng.randrange(R)), O.g2_mul(G2, rng.randrange(R))
    assert K.pairing_product([(p, q)]) == M.pairing(p, q)
    assert K.pairing_product([(G1, G2), (p, q), (None, q), (G1, G2)]) == M.f12_mul(M.f12_mul(e_gen, e_gen), M.pairing(p, q))
    assert K.pairing_product([]) == M.F12_ONE


def test_kernel_inversion_cells(e_gen):
    a = M.f12_mul(M.miller_loop(G1, G2), e_gen)
    m = K.Cells()
    m.copy(K.A, {i: c for i, c in enumerate(a[0] + a[1])}, 0, 6)
    K.x12_inv(m, K.C, K.A, K.SCR)
    assert M.f12_mul(K.cells_to_f12(m, K.C), a) == M.F12_ONE
    assert max(m) < 56  # kPairFinalCells (csrc/plans.hpp)


# ------------------------------------------------------------------------------------- the batch equation, model only
def test_batch_check_equation_in_the_model():
    """ark-poly-commit's batch_check for a synthetic setup with known tau and gamma (beta = tau)"""
    rng = random.Random(3)
    tau, gamma = rng.randrange(R), rng.randrange(R)
    ev = lambda c, x: sum(ci * pow(x, i, R) for i, ci in enumerate(c)) % R  # noqa: E731
    gamma_g, beta_h = O.g1_mul(G1, gamma), O.g2_mul(G2, tau)
    items = []
    for _ in range(3):
        p, b, z = [rng.randrange(R) for _ in range(4)], [rng.randrange(R) for _ in range(2)], rng.randrange(R)
        inv = pow((tau - z) % R, R - 2, R)
        c = O.g1_mul(G1, (ev(p, tau) + gamma * ev(b, tau)) % R)
        w = O.g1_mul(G1, ((ev(p, tau) - ev(p, z)) + gamma * (ev(b, tau) - ev(b, z))) * inv % R)
        items.append((c, z, ev(p, z), ev(b, z), w))
    rho = [1, rng.getrandbits(128), rng.getrandbits(128)]

    def accepted(items):
        total_c, total_w, sv, sb = None, None, 0, 0
        for r, (c, z, v, vb, w) in zip(rho, items):
            total_c = O.g1_add(total_c, O.g1_mul(O.g1_add(c, O.g1_mul(w, z)), r))
            total_w = O.g1_add(total_w, O.g1_mul(w, r))
            sv, sb = (sv + r * v) % R, (sb + r * vb) % R
        total_c = O.g1_add(total_c, O.g1_add(O.g1_mul(G1, -sv % R), O.g1_mul(gamma_g, -sb % R)))
        neg_w = (total_w[0], -total_w[1] % P)
        return M.pairing_product([(total_c, G2), (neg_w, beta_h)]) == M.F12_ONE

    assert accepted(items)
    c, z, v, vb, w = items[1]
    assert not accepted([items[0], (c, z, (v + 1) % R, vb, w), items[2]])
