"""The G1 subgroup test on the radix-2^30 ladders (csrc/curve.hpp jac<f30>) through the C ABI:
g1_decompress (fused and KZGPOT_SPLIT_PHASES) and g1_transcode at n = 1, 255, 257 and 4,096 (one
lane, a tail block, one block + 1, many blocks), on inputs built with the Python oracle:

  * subgroup points with both sign flags;
  * on-curve points outside the subgroup: random ones, pure cofactor torsion [r]Q, points of
    order 3 ([r h1 / 3]Q and (0, +-2)) and of order 11 ([r h1 / 11^2]Q: E(Fp)[11] is Z11 x Z11, so
    the whole 11-part of h1 but one factor is cleared), and sums G + T;
  * the ladder's exceptional branches: an order-3 point sends the ladder's first step (a tripling)
    to infinity, and an order-11 point meets the equal-point branch of the first mixed addition
    (|u| = 0b1101..: the accumulator is [12]P = P there);
  * rejected encodings mixed in.

Bytes, per-point status and first_bad are compared with the same call under KZGPOT_SUBGROUP_REF
(the reference's double-and-add by r, which stays on 14 x 28 limbs) and with the Python oracle."""
import random

import pytest

import kzgpot_oracle as O


REF, SPLIT = 0x2, 0x4
SIZES = [1, 255, 257, 4096]


def _torsion(rng, ell):
    e = 0
    while O.H1 % ell ** (e + 1) == 0:
        e += 1
    for _ in range(64):
        t = O.g1_mul(O.g1_random_on_curve(rng), O.R_ORDER * O.H1 // ell ** e)
        if t is not None:
            assert O.g1_mul(t, ell) is None
            return t
    raise AssertionError("no torsion point")


def _neg(pt):
    return pt[0], (-pt[1]) % O.P


@pytest.fixture(scope="module")
def pool():
    """[(compressed 48 B, pairing uncompressed 96 B | None)], the first entry a valid point"""
    rng = random.Random(30_13)
    pts = []
    for _ in range(4):
        g = O.g1_mul(O.G1_GEN, rng.randrange(1, O.R_ORDER))
        pts += [g, _neg(g)]
    t3, t11 = _torsion(rng, 3), _torsion(rng, 11)
    q = O.g1_random_on_curve(rng)
    pts += [q, _neg(q), O.g1_random_on_curve(rng), O.g1_mul(q, O.R_ORDER), O.g1_mul(O.g1_random_on_curve(rng), O.R_ORDER)]
    pts += [t3, _neg(t3), (0, 2), (0, O.P - 2), t11, _neg(t11), O.g1_mul(t11, 5), _torsion(rng, 11)]
    pts += [O.g1_add(pts[0], t3), O.g1_add(pts[1], t11), O.g1_add(pts[2], O.g1_add(t3, t11))]
    assert all(O.g1_on_curve(p) for p in pts)
    recs = [(O.pairing_g1_compress(p), O.pairing_g1_uncompressed(p)) for p in pts]
    # rejected encodings: compression bit clear, x >= p, a non-residue x^3 + 4, infinity
    good = recs[0][0]
    x = next(x for x in range(5, 200) if pow(x ** 3 + 4, (O.P - 1) // 2, O.P) != 1)
    bad = [bytes([good[0] & 0x7F]) + good[1:], bytes([0x80 | (O.P >> 376)]) + ((O.P + 5) & ((1 << 376) - 1)).to_bytes(47, "big"),
           bytes([0x80]) + x.to_bytes(47, "big"), bytes([0xC0]) + bytes(47)]
    recs += [(b, None) for b in bad]
    # transcode only: x >= p, and an off-curve (x, y + 1), which the reference tests by r all the same
    u = recs[0][1]
    off = u[:48] + ((int.from_bytes(u[48:], "big") + 1) % O.P).to_bytes(48, "big")
    recs += [(None, (O.P + 1).to_bytes(48, "big") + u[48:]), (None, off)]
    return recs


def _stream(pool, col, n):
    avail = [r[col] for r in pool if r[col] is not None]
    rng = random.Random(n)
    return [avail[0]] + [avail[rng.randrange(len(avail))] for _ in range(n - 1)]


_oracle_cache = {}


def _oracle(fn, recs, out_rec):
    out, sts, fb = bytearray(len(recs) * out_rec), [], -1
    for i, r in enumerate(recs):
        if (fn, r) not in _oracle_cache:
            _oracle_cache[(fn, r)] = fn(r)
        st, o = _oracle_cache[(fn, r)]
        sts.append(st)
        if st == O.OK:
            out[i * out_rec:(i + 1) * out_rec] = o
        elif fb < 0:
            fb = i
    return bytes(out), bytes(sts), fb


def _check(gpu, op, flags, recs, fn):
    data = b"".join(recs)
    got = gpu.run_codec(op, data, flags, want_status=True)
    ref = gpu.run_codec(op, data, flags | REF, want_status=True)
    assert (got.out, got.status, got.first_bad, got.ret) == (ref.out, ref.status, ref.first_bad, ref.ret)
    out, st, fb = _oracle(fn, recs, 96)
    assert got.status == st
    assert got.out == out
    assert got.first_bad == fb
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("flags", [0, SPLIT], ids=["fused", "split"])
def test_g1_decompress(gpu, pool, flags, n):
    st = _check(gpu, "g1_decompress", flags, _stream(pool, 0, n), O.g1_decompress_point)
    if n >= 255:
        assert {0, 1, 3, 4, 5, 7} <= set(st)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_g1_transcode(gpu, pool, n):
    st = _check(gpu, "g1_transcode", 0, _stream(pool, 1, n), O.g1_transcode_point)
    if n >= 255:
        assert {0, 3, 5} <= set(st)


def test_pool_decisions(pool):
    """what the pool is for: the oracle accepts exactly the 8 subgroup points (needs no GPU)"""
    sts = [O.g1_decompress_point(c)[0] for c, _ in pool if c is not None]
    assert sts[:8] == [0] * 8 and sts[8:24] == [5] * 16 and sts[24:] == [1, 3, 4, 7]
