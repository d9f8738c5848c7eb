"""Polynomial division over Fr on the GPU and the KZG10 open on top of it, exact.

The Fr reference is Python integer arithmetic: plain Horner for the quotient and the value. The
group reference is ONE oracle scalar multiplication per expected point, as in test_gpu_msm.py: the
bases are the golden transcript's setup (powers_of_g[j] = [tau^j]G, powers_of_gamma_g[j] =
[alpha tau^j]G with the known tau, alpha), so the proof's point is
    w = [ (p(tau) - p(z)) / (tau - z) + alpha (b(tau) - b(z)) / (tau - z) ] G
with the bracket computed by a field inverse, independent of the division algorithm. Every
comparison is bytes or integers."""
import random

import pytest

import kzgpot_oracle as O
from test_gpu_lagrange import ALPHA, TAU, g1_points
from test_gpu_msm import INF1, N, NG1, TAU_POW, poly_eval, powers, tau_g1, transcript  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

R = O.R_ORDER
TOP = (1 << 256) - 1
EDGE = [0, R - 1, R, R + 1, 2 * R + 1, TOP]


@pytest.fixture(scope="module")
def g1(oracle_lib):
    return lambda ks: g1_points(oracle_lib, ks)


def horner(coeffs, z):
    """(quotient, value) of the division by (x - z): q[j] = H[j + 1], value = H[0]."""
    h, acc = [0] * len(coeffs), 0
    for j in range(len(coeffs) - 1, -1, -1):
        acc = (acc * z + coeffs[j]) % R
        h[j] = acc
    return h[1:], (h[0] if h else 0)


def le(values):
    return b"".join(v.to_bytes(32, "little") for v in values)


def rand256(rng, n):
    return [rng.getrandbits(256) for _ in range(n)]


def check_divide(gpu, coeffs, z, tile=0):
    q, v = horner(coeffs, z)
    got_q, got_v = gpu.fr_poly_divide(coeffs, z, tile=tile)
    assert got_v == v
    assert got_q == le(q)
    assert gpu.fr_poly_divide(coeffs, z, tile=tile, want_quotient=False) == (None, v)


# ------------------------------------------------------------------------------------- 1: the division kernels alone
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65537])
def test_divide_sizes(gpu, n):
    rng = random.Random(n)
    check_divide(gpu, rand256(rng, n), rng.getrandbits(256))


@pytest.mark.parametrize("n", [511, 513, 65537, 131071])
def test_divide_tile_8_levels(gpu, n):
    """Tiles of 256: 65,537 = 256^2 + 1 coefficients are two full levels and the first entry of a third."""
    rng = random.Random(8000 + n)
    check_divide(gpu, rand256(rng, n), rng.getrandbits(256), tile=8)


def test_evaluate(gpu):
    rng = random.Random(21)
    c, z = rand256(rng, 5000), rng.getrandbits(256)
    assert gpu.kzg_evaluate(c, z) == poly_eval(c, z) == horner(c, z)[1]
    assert gpu.kzg_evaluate([], z) == 0
    assert gpu.kzg_evaluate([R + 7], z) == 7


@pytest.mark.parametrize("z", [0, 1, R - 1, R, TOP, random.Random(3).getrandbits(256)],
                         ids=["0", "1", "r-1", "r", "2^256-1", "random"])
def test_divide_points(gpu, z):
    c = rand256(random.Random(31), 1000)
    check_divide(gpu, c, z, tile=8)  # four tiles, two levels
    check_divide(gpu, c, z)


def test_divide_edge_coefficients(gpu):
    rng = random.Random(41)
    c = EDGE + rand256(rng, 290) + EDGE[::-1]
    for z in (rng.getrandbits(256), TOP, 0):
        check_divide(gpu, c, z, tile=8)
    check_divide(gpu, EDGE, 2)
    check_divide(gpu, [R, 2 * R, 0, R], 5)  # the zero polynomial, unreduced
    for a in EDGE:
        assert gpu.fr_poly_divide([a], 3) == (b"", a % R)


def test_divide_by_a_root(gpu):
    """p(x) = (x - z) s(x): the value is 0 and the quotient is s."""
    rng = random.Random(51)
    z = rng.randrange(R)
    s = [rng.randrange(R) for _ in range(700)]
    p = [(a - z * b) % R for a, b in zip([0] + s, s + [0])]
    for tile in (0, 8):
        assert gpu.fr_poly_divide(p, z, tile=tile) == (le(s), 0)


def test_quotient_does_not_depend_on_the_tile(gpu):
    rng = random.Random(61)
    c, z = rand256(rng, 5000), rng.getrandbits(256)
    q, v = horner(c, z)
    for tile in (0, 8, 9, 10, 11, 12):
        assert gpu.fr_poly_divide(c, z, tile=tile) == (le(q), v), tile


# ------------------------------------------------------------------------------------- 2: open against the trapdoor
def witness_scalar(p, b, z):
    """(p(tau) - p(z)) / (tau - z) + alpha (b(tau) - b(z)) / (tau - z) mod r, by a field inverse"""
    inv = pow((TAU - z) % R, R - 2, R)
    wp = (poly_eval(p, TAU) - poly_eval(p, z)) * inv
    wb = (poly_eval(b, TAU) - poly_eval(b, z)) * inv
    return (wp + ALPHA * wb) % R


def check_open(gpu, g1, powers, p, b, z, **kw):
    proof = gpu.kzg_open(powers, p, z, blinding=b, **kw)
    w = witness_scalar(p, b or [], z)
    assert proof.w == g1([w])
    assert proof.value == poly_eval(p, z)
    assert proof.random_v == (poly_eval(b, z) if b is not None else None)
    # the check equation in the exponent: C = [w (tau - z) + value + alpha random_v] G
    rv = proof.random_v or 0
    assert gpu.kzg_commit(powers, p, b) == g1([(w * (TAU - z) + proof.value + ALPHA * rv) % R])
    return proof


def test_open_reference_shape(gpu, g1, powers):
    """end_to_end_test_kzg's own shape: degrees 2 .. 19, hiding with a 3-coefficient blinding
    polynomial, ten polynomials."""
    rng = random.Random(71)
    for _ in range(10):
        p = [rng.randrange(R) for _ in range(rng.randrange(2, 20) + 1)]
        b = [rng.randrange(R) for _ in range(3)]
        check_open(gpu, g1, powers, p, b, rng.randrange(R))


def test_open_not_hiding(gpu, g1, powers):
    rng = random.Random(72)
    p = [rng.randrange(R) for _ in range(20)]
    proof = check_open(gpu, g1, powers, p, None, rng.randrange(R))
    assert proof.random_v is None


def test_open_both_ranges_to_their_ends(gpu, g1, powers):
    rng = random.Random(73)
    p = [rng.randrange(R) for _ in range(N)]
    b = [rng.randrange(R) for _ in range(N)]
    check_open(gpu, g1, powers, p, b, rng.randrange(R))
    check_open(gpu, g1, powers, p, b, rng.randrange(R), tile=8, window=5)


def test_open_all_powers(gpu, g1, powers):
    rng = random.Random(74)
    p = [rng.randrange(R) for _ in range(NG1)]  # degree 2,046
    check_open(gpu, g1, powers, p, None, rng.randrange(R))


def test_open_trivial_and_trimmed(gpu, g1, powers):
    z = 12345
    assert gpu.kzg_open(powers, [], z) == gpu.KzgProof(INF1, None, 0)
    assert gpu.kzg_open(powers, [R + 9], z) == gpu.KzgProof(INF1, None, 9)
    assert gpu.kzg_open(powers, [9], z, blinding=[4]) == gpu.KzgProof(INF1, 4, 9)
    rng = random.Random(75)
    p = [rng.randrange(R) for _ in range(12)]
    b = [rng.randrange(R) for _ in range(3)]
    want = check_open(gpu, g1, powers, p, b, z)
    assert gpu.kzg_open(powers, p + [0, R, 0], z, blinding=b + [0]) == want
    long_p = p + [0] * (NG1 + 5 - len(p))  # fits once trimmed
    assert gpu.kzg_open(powers, long_p, z, blinding=b) == want
    with pytest.raises(ValueError):
        gpu.kzg_open(powers, [1] * (NG1 + 1), z)
    with pytest.raises(ValueError):
        gpu.kzg_open(powers, p, z, blinding=[1] * (N + 1))


# ------------------------------------------------------------------------------------- 3: record forms, malformed bases
@pytest.fixture(scope="module")
def ark_setup(g1, tau_g1):
    """ark-uncompressed records of the first 16 powers_of_g and powers_of_gamma_g"""
    return tau_g1[: 96 * 16], g1([ALPHA * t % R for t in TAU_POW[:16]])


def test_ark_and_montgomery_bases(gpu, g1, powers, ark_setup):
    pg, pgg = ark_setup
    rng = random.Random(81)
    p, b, z = rand256(rng, 12), rand256(rng, 5), rng.getrandbits(256)
    ark = gpu.g1_kzg_open(pg, p, pgg, b, z)
    assert (ark.ret, ark.first_bad, len(ark.out)) == (0, -1, 160)
    mont = gpu.g1_kzg_open(powers.powers_of_g[:11].tobytes(), p, powers.powers_of_gamma_g[:4].tobytes(), b, z,
                           mont=True)
    assert mont == ark
    pr, br, zr = [c % R for c in p], [c % R for c in b], z % R
    assert ark.out == g1([witness_scalar(pr, br, zr)]) + le([poly_eval(pr, zr), poly_eval(br, zr)])
    for tile, window in ((8, 3), (12, 16)):
        assert gpu.g1_kzg_open(pg, p, pgg, b, z, tile=tile, window=window) == ark


def test_malformed_bases(gpu, ark_setup):
    pg, pgg = ark_setup
    rng = random.Random(82)
    p, b, z = rand256(rng, 12), rand256(rng, 5), rng.getrandbits(256)
    bad = bytearray(pg)
    bad[5 * 96: 5 * 96 + 48] = (O.P + 5).to_bytes(48, "little")
    r = gpu.g1_kzg_open(bytes(bad), p, pgg, b, z)
    assert (r.ret, r.first_bad, r.out) == (-3, 5, b"")
    bad = bytearray(pgg)
    bad[1 * 96: 1 * 96 + 48] = O.P.to_bytes(48, "little")
    r = gpu.g1_kzg_open(pg, p, bytes(bad), b, z)
    assert (r.ret, r.first_bad, r.out) == (-3, len(p) - 1 + 1, b"")
    # records past the n - 1 and n_blind - 1 that open reads are not looked at
    bad = bytearray(pg)
    bad[11 * 96: 11 * 96 + 48] = O.P.to_bytes(48, "little")
    assert gpu.g1_kzg_open(bytes(bad), p, pgg, b, z) == gpu.g1_kzg_open(pg, p, pgg, b, z)


# ------------------------------------------------------------------------------------- 4: device entries, side stream
def test_dev_on_a_side_stream(gpu, ark_setup):
    import torch
    from kzgpot import device as D

    pg, pgg = ark_setup
    rng = random.Random(91)
    p, b, z = rand256(rng, 14), rand256(rng, 3), rng.getrandbits(256)
    want = gpu.g1_kzg_open(pg, p, pgg, b, z)
    assert want.ret == 0
    dev = torch.device("cuda:0")
    to_dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    d_pg, d_pgg, d_p, d_b = to_dev(pg), to_dev(pgg), to_dev(le(p)), to_dev(le(b))
    out = torch.full((160,), 0xAB, dtype=torch.uint8, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work = D.g1_kzg_open_dev(d_pg, d_p, z, out, key, d_powers_of_gamma_g=d_pgg, d_blinding=d_b)
    side.synchronize()
    assert work.numel() == gpu.kzg_open_workspace(len(p), len(b))
    assert D.read_key(key) == (1 << 64) - 1
    assert bytes(out.cpu().numpy()) == want.out

    for where, index in ((d_pg, 5), (d_pgg, 1)):
        bad = where.clone()
        bad[index * 96: index * 96 + 48] = to_dev((O.P + 1).to_bytes(48, "little"))
        args = (bad, d_pgg) if where is d_pg else (d_pg, bad)
        out.fill_(0xAB)
        D.g1_kzg_open_dev(args[0], d_p, z, out, key, d_powers_of_gamma_g=args[1], d_blinding=d_b, work=work)
        torch.cuda.synchronize()
        first_bad = index if where is d_pg else len(p) - 1 + index
        assert D.read_key(key) == (first_bad << 8) | 3
        assert bytes(out.cpu().numpy()) == b"\xab" * 160

    # the division's own device entry, device-resident coefficients, evaluate-only included
    c = rand256(rng, 3000)
    q, v = horner(c, z % R)
    d_c = to_dev(le(c))
    d_q = torch.full((32 * 2999,), 0xAB, dtype=torch.uint8, device=dev)
    d_v = torch.full((64,), 0xAB, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(side):
        work = D.fr_poly_divide_dev(d_c, z, d_q, d_v[:32], tile=9)
        D.fr_poly_divide_dev(d_c, z, None, d_v[32:], tile=9, work=work)
    side.synchronize()
    assert work.numel() == gpu.fr_poly_workspace(3000, 9 << 16)
    assert bytes(d_q.cpu().numpy()) == le(q)
    assert bytes(d_v.cpu().numpy()) == le([v, v])
