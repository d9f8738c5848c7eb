"""Limb / value bounds of the multi-scalar multiplication (csrc/msm_kernels.hip), with
tests/field_bounds_model.py unchanged.

k_msm_sum chains jac_madd without a doubling in between, which the ladder bound set of
test_field_bounds.py does not cover. The kernel therefore brings X, Y and Z back through fp_canon
after every addition, and what is shown here without a BoundError is one link of that chain:
  * jac_madd from a canonical accumulator (X, Y, Z each < p, limbs < 2^28) and from Z = 0 (the
    empty sum) with a canonical base — M.jac_madd joins the equal-point branch's jac_dbl outputs
    into its result, and jac_dbl from the same inputs is run on its own as well — every output
    passing fp_canon's input condition;
  * the normalisation of a chunk's sum and of the final result: group_parts.hpp's
    canon_jac_to_affine, as test_field_bounds_lagrange.py states it once per field;
  * k_msm_final's ladder: jac_dbl, then jac_madd of a canonical base — the proven ladder set, from
    Z = 0, its states canonicalised at the end;
  * k_msm_load's two inputs: a range-checked coordinate to Montgomery form (as k_fft_load), and an
    ark-ff Montgomery image (R = 2^384, < p) times FP_FROM_ARK = 2^400 mod p."""
import field_bounds_model as M
from test_field_bounds_lagrange import _v2, canon, canon_jac_to_affine_fp, canon_jac_to_affine_fp2, canonical, reduce_once


def zero():
    return M.normalized(0, "zero")


def test_g1_chained_addition_link():
    base = canonical("base")
    for Z in (canonical("Z"), zero()):
        acc = (canonical("X"), canonical("Y"), Z)
        for v in M.jac_madd(*acc, base, base):
            canon(v, "madd")
        for v in M.jac_dbl(*acc):
            canon(v, "dbl")
    # empty sum: X = Y = Z = 0
    for v in M.jac_madd(zero(), zero(), zero(), base, base):
        canon(v, "madd from the empty sum")


def test_g2_chained_addition_link():
    base = _v2(canonical("base"))
    for Z in (_v2(canonical("Z")), _v2(zero())):
        acc = (_v2(canonical("X")), _v2(canonical("Y")), Z)
        for v in M.jac_madd_fp2(*acc, base, base):
            canon(v.c0, "madd.c0"), canon(v.c1, "madd.c1")
        for v in M.jac_dbl_fp2(*acc):
            canon(v.c0, "dbl.c0"), canon(v.c1, "dbl.c1")
    for v in M.jac_madd_fp2(_v2(zero()), _v2(zero()), _v2(zero()), base, base):
        canon(v.c0, "madd.c0"), canon(v.c1, "madd.c1")


def test_g1_normalisation():
    """A chunk's sum (k_msm_sum) and the final result (k_msm_final): the shared tail."""
    canon_jac_to_affine_fp(canonical("X"), canonical("Y"), canonical("Z"))


def test_g2_normalisation():
    X = Y = Z = _v2(canonical())
    canon_jac_to_affine_fp2(X, Y, Z)


def test_final_ladder_is_the_proven_set():
    base = canonical("T_k")
    S = M.ladder_invariant(base, base)
    for v in S:
        canon(v, "final")
    base2 = _v2(canonical("T_k"))
    for v in M.ladder_invariant_fp2(base2, base2):
        canon(v.c0, "final.c0"), canon(v.c1, "final.c1")
    # the ladder starts from X = Y = Z = 0, below every bound of S
    assert all(z <= s for v in S for z, s in zip(zero().limbs, v.limbs))


def test_load_conversions():
    reduce_once(M.mul(canonical("x"), canonical("R2"), "to_mont"), "ark record")
    reduce_once(M.mul(canonical("x 2^384"), canonical("FP_FROM_ARK"), "from_ark"), "GroupAffine record")
    consts = open(M.CONSTS).read()
    limbs = [int(t.rstrip("u"), 16) for t in consts.split("FP_FROM_ARK[14] = {")[1].split("}")[0].split(", ")]
    value = sum(v << (M.LB * i) for i, v in enumerate(limbs))
    assert value == (1 << 400) % M.P and all(v <= M.LM for v in limbs)
    # x 2^384 times 2^400 / 2^392 = x 2^392: the internal Montgomery form
    assert value * (1 << 384) % M.P == (1 << 784) % M.P
