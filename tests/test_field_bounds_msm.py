"""Limb / value bounds of the multi-scalar multiplication (csrc/msm_kernels.hip), with
tests/field_bounds_model.py unchanged.

k_msm_sum chains jac_madd without a doubling in between, which the ladder bound set of
test_field_bounds.py does not cover. The kernel therefore brings X, Y and Z back through fp_canon
after every addition, and what is shown here without a BoundError is one link of that chain:
  * jac_madd from a canonical accumulator (X, Y, Z each < p, limbs < 2^28) and from Z = 0 (the
    empty sum) with a canonical base — M.jac_madd joins the equal-point branch's jac_dbl outputs
    into its result, and jac_dbl from the same inputs is run on its own as well — every output
    passing fp_canon's input condition;
  * the normalisation of a chunk's sum and of the final result: inversion of a canonical Z,
    x = X z^-2, y = Y z^-3, one conditional subtraction each, and the emit's from-Montgomery input;
  * k_msm_final's ladder: jac_dbl, then jac_madd of a canonical base — the proven ladder set, from
    Z = 0, its states canonicalised at the end;
  * k_msm_load's two inputs: a range-checked coordinate to Montgomery form (as k_fft_load), and an
    ark-ff Montgomery image (R = 2^384, < p) times FP_FROM_ARK = 2^400 mod p."""
import field_bounds_model as M
from test_field_bounds_lagrange import _v2, canon, canonical, inv_fp, inv_fp2, reduce_once, reduce_once2


def zero():
    return M.normalized(0, "zero")


def test_g1_chained_addition_link():
    F = M.Field(False)
    base = canonical("base")
    for Z in (canonical("Z"), zero()):
        acc = (canonical("X"), canonical("Y"), Z)
        for v in M.jac_madd(F, *acc, base, base):
            canon(v, "madd")
        for v in M.jac_dbl(F, *acc):
            canon(v, "dbl")
    # empty sum: X = Y = Z = 0
    for v in M.jac_madd(F, zero(), zero(), zero(), base, base):
        canon(v, "madd from the empty sum")


def test_g2_chained_addition_link():
    base = _v2(canonical("base"))
    for Z in (_v2(canonical("Z")), _v2(zero())):
        acc = (_v2(canonical("X")), _v2(canonical("Y")), Z)
        for v in M.jac_madd_fp2_lz(*acc, base, base):
            canon(v.c0, "madd.c0"), canon(v.c1, "madd.c1")
        for v in M.jac_dbl_fp2_lz(*acc):
            canon(v.c0, "dbl.c0"), canon(v.c1, "dbl.c1")
    for v in M.jac_madd_fp2_lz(_v2(zero()), _v2(zero()), _v2(zero()), base, base):
        canon(v.c0, "madd.c0"), canon(v.c1, "madd.c1")


def test_g1_normalisation():
    X, Y, Z = canonical("X"), canonical("Y"), canonical("Z")
    zi = reduce_once(inv_fp(Z), "1/Z")
    z2 = M.sqr(zi, "zi2")
    x = reduce_once(M.mul(X, z2, "x"), "x")
    y = reduce_once(M.mul(Y, M.mul(z2, zi, "zi3"), "y"), "y")
    M.from_mont_ok(x, "emit x"), M.from_mont_ok(y, "emit y")


def test_g2_normalisation():
    X = Y = Z = _v2(canonical())
    zi = reduce_once2(inv_fp2(Z), "1/Z")
    z2 = M.f2_sqr(zi, "zi2")
    x = reduce_once2(M.f2_mul(X, z2, "x"))
    y = reduce_once2(M.f2_mul(Y, M.f2_mul(z2, zi, "zi3"), "y"))
    for c in (x.c0, x.c1, y.c0, y.c1):
        M.from_mont_ok(c, "emit")


def test_final_ladder_is_the_proven_set():
    F = M.Field(False)
    base = canonical("T_k")
    S = M.ladder_invariant(F, base, base)
    for v in S:
        canon(v, "final")
    base2 = _v2(canonical("T_k"))
    for v in M.ladder_invariant_fp2_lz(base2, base2):
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
