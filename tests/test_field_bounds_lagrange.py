"""Limb / value bounds of the group FFT's butterfly (csrc/fft_kernels.hip k_fft_stage, k_h_bases,
k_fft_point_mul, k_fft_emit), with tests/field_bounds_model.py unchanged.

The ladder [w]Q is jac_dbl + jac_madd from a canonical base, so its states lie in the ladder bound
set S that test_field_bounds.py proves closed under "double, then optionally add the base" for any
bit pattern (Z = 0, the ladder's start, is below every bound). What the butterfly adds, and what is
shown here for ANY element of S without a BoundError:
  * the final mixed additions T + P and T + (-P) with a canonical P (S is only proven closed under
    double-then-add), whose outputs — and T itself when P is infinite — go through fp_canon;
  * -P's y as fp_neg_canon of a canonical value (canonical again);
  * the shared inversion 1 / (Z0 Z1) and the two affine conversions, all on canonical values in the
    reduced discipline, each product brought back below p by one conditional subtraction;
  * the emit's from-Montgomery input and the load's to-Montgomery output."""
from fractions import Fraction

import field_bounds_model as M


def canonical(name="canonical"):
    return M.normalized(1, name)  # value < p, limbs < 2^28


def reduce_once(a, name="reduce_once"):
    """fp_reduce_once: normalized, value < 2p -> canonical."""
    M.reduce_once_ok(a, name)
    return canonical(name)


def canon(a, name="canon"):
    """fp_canon: limbs < 2^32 - 16, value < 256 p -> canonical."""
    M.canon_ok(a, name)
    return canonical(name)


def neg_canon(a, name="neg_canon"):
    """fp_neg_canon: p - a limb by limb with a borrow chain; a must be canonical."""
    assert a.val <= 1 + 1e-6 and all(l <= M.LM for l in a.limbs), a
    return canonical(name)


def pow_pm3d4(a):
    """fp_pow_pm3d4 (BLS12-381: the radix-2^30 chain): any input with limbs < 2^32 - 16 and value
    < 2^383; output normalized, value < 1.01 p (as test_field_bounds._pow_pm3d4)."""
    assert max(a.limbs) < (1 << 32) - 16 and a.val * M.P < 2 ** 383, a
    return M.normalized(Fraction(101, 100))


def inv_fp(a, name="inv"):
    """curve.hpp f_inv(fp): t = a^((p-3)/4), t^4 a."""
    t = pow_pm3d4(a)
    t = M.sqr(M.sqr(t, name + ".t2"), name + ".t4")
    return M.mul(t, a, name)


def scale_to_affine_fp(X, Y, zi):
    """group_parts.hpp scale_to_affine over Fp: canonical X, Y, zi -> canonical x, y."""
    z2 = M.sqr(zi, "zi2")
    x = reduce_once(M.mul(X, z2, "x"), "x")
    z3 = M.mul(z2, zi, "zi3")
    y = reduce_once(M.mul(Y, z3, "y"), "y")
    return x, y


def canon_jac_to_affine_fp(X, Y, Z):
    """group_parts.hpp canon_jac_to_affine over Fp, the one Jacobian -> affine tail of the scale /
    per-point pass (k_fft_point_mul), k_h_bases, k_msm_sum and k_msm_final: canonical X, Y and Z
    (an infinite Z replaced by the canonical 1), one inversion, scale_to_affine; the result is
    canonical and fits the emit's from-Montgomery input."""
    zi = reduce_once(inv_fp(Z), "1/Z")
    x, y = scale_to_affine_fp(X, Y, zi)
    M.from_mont_ok(x, "emit x"), M.from_mont_ok(y, "emit y")
    return x, y


def test_g1_butterfly_bounds():
    base = M.normalized(Fraction(101, 100))  # the work buffer holds canonical values: a subset
    S = M.ladder_invariant(base, base)
    M.jac_eq_affine(*S, base, base)  # the set test_field_bounds.py proves
    for v in S:  # T itself is canonicalised when P is infinite, and in the scale / per-point pass
        canon(v, "T")
    canon_jac_to_affine_fp(canonical("T.X"), canonical("T.Y"), canonical("T.Z"))  # k_fft_point_mul
    ny = neg_canon(canonical("P.y"))
    for py in (canonical("P.y"), ny):  # R0 = T + P, R1 = T + (-P), from any ladder state
        R = M.jac_madd(*S, canonical("P.x"), py)
        X, Y, Z = (canon(v, "R") for v in R)
    # one inversion for both results
    z0, z1 = canonical("Z0"), canonical("Z1")
    zz = reduce_once(M.mul(z0, z1, "Z0Z1"))
    zi = reduce_once(inv_fp(zz), "1/(Z0Z1)")
    zi0 = reduce_once(M.mul(zi, z1, "zi0"))
    zi1 = reduce_once(M.mul(zi, z0, "zi1"))
    for z in (zi0, zi1):
        x, y = scale_to_affine_fp(X, Y, z)
        M.from_mont_ok(x, "emit x")  # k_fft_emit
        M.from_mont_ok(neg_canon(y, "-y"), "emit y")  # out1's y is negated (P - T = -(T - P))


def test_g1_load_and_h_bases_bounds():
    """k_fft_load: a range-checked coordinate (< p) to Montgomery form and one conditional
    subtraction. k_h_bases: (x, y, 1) + (x', -y') from records of a checked decode, then the
    single-point inversion."""
    xm = M.mul(canonical("x"), canonical("R2"), "to_mont")
    reduce_once(xm, "load")
    R = M.jac_madd(xm, xm, M.normalized(1), xm, neg_canon(reduce_once(xm)))
    canon_jac_to_affine_fp(*(canon(v, "h") for v in R))


def _v2(v):
    return M.V2(v, v)


def inv_fp2(a):
    """curve.hpp f_inv(fp2): (a0 - a1 u) / (a0^2 + a1^2), reduced in and out."""
    n = M.norm(M.add_nr(M.sqr(a.c0, "a0^2"), M.sqr(a.c1, "a1^2"), "norm"))
    n = inv_fp(n, "1/norm")
    c0 = M.mul(a.c0, n, "inv.c0")
    c1 = M.sub_red(M.normalized(0), M.mul(a.c1, n, "inv.t"), "inv.c1")
    return M.V2(c0, c1)


def reduce_once2(a, name="reduce_once2"):
    return M.V2(reduce_once(a.c0, name), reduce_once(a.c1, name))


def scale_to_affine_fp2(X, Y, zi):
    """group_parts.hpp scale_to_affine over Fp2, in the reduced discipline (f_mul / f_sqr)."""
    z2 = M.f2_sqr(zi, "zi2")
    x = reduce_once2(M.f2_mul(X, z2, "x"))
    z3 = M.f2_mul(z2, zi, "zi3")
    y = reduce_once2(M.f2_mul(Y, z3, "y"))
    return x, y


def canon_jac_to_affine_fp2(X, Y, Z):
    """group_parts.hpp canon_jac_to_affine over Fp2: as canon_jac_to_affine_fp, per component."""
    zi = reduce_once2(inv_fp2(Z), "1/Z")
    x, y = scale_to_affine_fp2(X, Y, zi)
    for c in (x.c0, x.c1, y.c0, y.c1):
        M.from_mont_ok(c, "emit")
    return x, y


def test_g2_butterfly_bounds():
    base = _v2(M.normalized(Fraction(101, 100)))
    S = M.ladder_invariant_fp2(base, base)
    M.jac_eq_affine_fp2(*S, base, base)
    for v in S:
        canon(v.c0, "T.c0"), canon(v.c1, "T.c1")
    T = _v2(canonical("T"))
    canon_jac_to_affine_fp2(T, T, T)  # k_fft_point_mul
    P = _v2(canonical("P"))
    nP = M.V2(neg_canon(P.c0), neg_canon(P.c1))
    for py in (P, nP):
        R = M.jac_madd_fp2(*S, P, py)
        for v in R:
            canon(v.c0, "R.c0"), canon(v.c1, "R.c1")
    # the tail runs on canonical values in the reduced Fp2 discipline (f_mul / f_sqr / f_inv)
    X = Y = z0 = z1 = _v2(canonical())
    zz = reduce_once2(M.f2_mul(z0, z1, "Z0Z1"))
    zi = reduce_once2(inv_fp2(zz), "1/(Z0Z1)")
    zi0 = reduce_once2(M.f2_mul(zi, z1, "zi0"))
    x, y = scale_to_affine_fp2(X, Y, zi0)
    for c in (x.c0, x.c1, neg_canon(y.c0), neg_canon(y.c1)):
        M.from_mont_ok(c, "emit")
    # k_fft_load: as for G1, per component
    reduce_once(M.mul(canonical("x"), canonical("R2"), "to_mont"), "load")
