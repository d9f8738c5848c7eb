"""Fr vectors in evaluation form on the GPU, exact: the batch inversion, the division
by (x - z) from evaluations, and the KZG10 open on top of it.

The Fr reference shares no formula with the kernels. Inverses are pow(a, r - 2, r). For the
division, random coefficients go through a Python NTT to make `evals`; the value is Horner on the
coefficients and the quotient's evaluations are the same Python NTT of the Horner quotient's
coefficients: no barycentric sum, no inverted difference, no special case on the domain. The group
reference is ONE oracle scalar multiplication [(p(tau) - p(z)) / (tau - z)]G over the golden
transcript's known tau, as in test_gpu_poly_open.py, and the coefficient route (kzg_open, kzg_open_domain)
byte for byte. Every comparison is bytes or integers."""
import functools
import random

import pytest

import kzgpot_oracle as O
from test_gpu_lagrange import TAU, g1_points, omega
from test_gpu_msm import INF1, poly_eval, powers, tau_g1, transcript  # noqa: F401  (fixtures)
from test_gpu_poly_open import horner, le
from test_ntt_units import ntt_ref

pytestmark = pytest.mark.gpu

R = O.R_ORDER
TOP = (1 << 256) - 1
DEFAULT_TILE = 11  # kPolyTile (csrc/plans.hpp): what tile=0 selects


@pytest.fixture(scope="module")
def g1(oracle_lib):
    return lambda ks: g1_points(oracle_lib, ks)


def ints(data):
    return [int.from_bytes(data[o: o + 32], "little") for o in range(0, len(data), 32)]


# ------------------------------------------------------------------------------------- 1: batch inversion
def inverses(values):
    return [pow(v % R, R - 2, R) for v in values]


def check_inverse(gpu, values, tile=0):
    want = le(inverses(values))
    assert gpu.fr_batch_inverse(values, tile=tile) == want
    return want


@pytest.mark.parametrize("n", [0, 1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 65537])
def test_inverse_sizes(gpu, n):
    rng = random.Random(n)
    check_inverse(gpu, [rng.getrandbits(256) for _ in range(n)])


@pytest.mark.parametrize("tile", [8, 12])
@pytest.mark.parametrize("n", [511, 513, 4097])
def test_inverse_tiles(gpu, n, tile):
    rng = random.Random(100 * tile + n)
    check_inverse(gpu, [rng.getrandbits(256) for _ in range(n)], tile=tile)


@pytest.mark.parametrize("tile", [0, 8, 12])
def test_inverse_zeros(gpu, tile):
    """Zeros (0 and its unreduced forms) at both ends, on both sides of a run boundary and of a tile
    boundary, a whole run, a whole tile, everything."""
    t = tile or DEFAULT_TILE
    S, M = 1 << t, (1 << t) // 256
    n = 2 * S + 37
    rng = random.Random(200 + tile)
    base = [rng.randrange(1, R) for _ in range(n)]
    base_inverse = inverses(base)  # once: a zero changes no other entry's inverse
    zero = [0, R, 2 * R]
    for at in ([0], [n - 1], [0, n - 1], [M - 1], [M], [M - 1, M], [S - 1], [S], [S - 1, S],
               range(3 * M, 4 * M), range(S, 2 * S), range(2 * S, n)):
        v, want = list(base), list(base_inverse)
        for j, i in enumerate(at):
            v[i], want[i] = zero[j % 3], 0
        assert gpu.fr_batch_inverse(v, tile=tile) == le(want), (tile, list(at)[:2])
    assert gpu.fr_batch_inverse([0, R, 2 * R] * 100, tile=tile) == bytes(32 * 300)


def test_inverse_unreduced_inputs(gpu):
    rng = random.Random(31)
    edge = [R, R + 1, 2 * R + 1, TOP, 1, R - 1, 2, 2 * R]
    v = edge + [rng.getrandbits(256) for _ in range(300)] + edge[::-1]
    got = ints(check_inverse(gpu, v, tile=8))
    assert got[:4] == [0, 1, 1, pow(TOP % R, R - 2, R)] and got[5] == R - 1
    assert all(g * (x % R) % R == (1 if x % R else 0) for g, x in zip(got, v))


def test_inverse_does_not_depend_on_the_tile(gpu):
    rng = random.Random(41)
    v = [rng.getrandbits(256) for _ in range(5000)]
    for i in (0, 17, 2047, 2048, 4999):
        v[i] = 0
    want = le(inverses(v))
    for tile in (0, 8, 9, 10, 11, 12):
        assert gpu.fr_batch_inverse(v, tile=tile) == want, tile


def test_inverse_in_place_on_a_side_stream(gpu):
    import torch
    from kzgpot import device as D

    dev = torch.device("cuda:0")
    rng = random.Random(51)
    v = [rng.getrandbits(256) for _ in range(3000)]
    v[5] = v[2999] = 0
    want = le(inverses(v))
    d = torch.frombuffer(bytearray(le(v)), dtype=torch.uint8).to(dev)
    out = torch.full((32 * 3000 + 64,), 0xAB, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        D.fr_batch_inverse_dev(d, out, tile=9)  # apart
        D.fr_batch_inverse_dev(d, d, tile=9)    # in place
    side.synchronize()
    assert bytes(d.cpu().numpy()) == want
    assert bytes(out.cpu().numpy()) == want + b"\xab" * 64  # nothing past the last entry


# ------------------------------------------------------------------------------------- 2: division in evaluation form
@functools.lru_cache(maxsize=None)
def polynomial(exp, seed=0):
    """(coefficients, evaluations) of a random polynomial with 2^exp coefficients, computed once."""
    rng = random.Random(1000 * seed + exp)
    c = [rng.randrange(R) for _ in range(1 << exp)]
    return c, ntt_ref(c, exp)


def reference(coeffs, exp, z):
    """(the quotient's evaluations, the value): Horner, then the NTT of the quotient's coefficients."""
    q, v = horner(coeffs, z % R)
    return ntt_ref(q + [0], exp), v


def check_evals_divide(gpu, coeffs, evals, exp, z, tile=0):
    q, v = reference(coeffs, exp, z)
    got_q, got_v = gpu.fr_evals_divide(evals, exp, z, tile=tile)
    assert got_v == v, (exp, hex(z), tile)
    assert got_q == le(q), (exp, hex(z), tile)
    assert gpu.fr_evals_divide(evals, exp, z, tile=tile, want_quotient=False) == (None, v)
    assert gpu.kzg_evaluate_evals(evals, exp, z) == v


def points(exp, tile):
    """z off the domain (random, 0, r = 0, 2^256 - 1) and the w^m on it next to the run and tile boundaries."""
    n, t = 1 << exp, tile or DEFAULT_TILE
    M = (1 << t) // 256
    ms = sorted({m for m in (0, 1, n - 1, M - 1, M, (1 << t) - 1, 1 << t) if m < n})
    return [random.Random(exp).getrandbits(256), 0, R, TOP] + [pow(omega(exp), m, R) for m in ms]


@pytest.mark.parametrize("exp", [0, 1, 2, 7, 8, 9, 12, 13])
def test_evals_divide(gpu, exp):
    """The library's tile: below a wave, below a block, below a tile, two and four tiles."""
    c, e = polynomial(exp)
    for z in points(exp, 0):
        check_evals_divide(gpu, c, e, exp, z)


@pytest.mark.parametrize("exp", [10, 11, 13])
def test_evals_divide_small_and_exact_tiles(gpu, exp):
    """Tile 8: four and 32 tiles feed the two reductions. 2^11 at the library's tile: exactly one tile."""
    c, e = polynomial(exp)
    tile = 0 if exp == 11 else 8
    for z in points(exp, tile):
        check_evals_divide(gpu, c, e, exp, z, tile=tile)


def test_evals_divide_edge_evaluations(gpu):
    """Evaluations 0, r - 1 and the unreduced r, 2^256 - 1 among random 256-bit integers."""
    exp = 9
    rng = random.Random(61)
    e = [rng.getrandbits(256) for _ in range(1 << exp)]
    edge = [0, R - 1, R, TOP]
    e[:4], e[-4:], e[255:259] = edge, edge[::-1], edge
    c = ntt_ref(e, exp, inverse=True)
    assert ntt_ref(c, exp) == [v % R for v in e]
    for tile in (0, 8):
        for z in points(exp, tile)[:1] + [1, pow(omega(exp), 256, R), pow(omega(exp), 511, R)]:
            check_evals_divide(gpu, c, e, exp, z, tile=tile)


def test_evals_divide_constant_polynomial(gpu):
    exp = 9
    e = [R + 5] * (1 << exp)
    for z in (77, pow(omega(exp), 3, R)):
        assert gpu.fr_evals_divide(e, exp, z, tile=8) == (bytes(32 << exp), 5)
    assert gpu.fr_evals_divide([0] * 4, 2, 9) == (bytes(128), 0)


def test_evals_divide_does_not_depend_on_the_tile(gpu):
    exp = 12
    c, e = polynomial(exp)
    for z in (random.Random(71).getrandbits(256), pow(omega(exp), 2049, R)):
        q, v = reference(c, exp, z)
        for tile in (0, 8, 9, 10, 11, 12):
            assert gpu.fr_evals_divide(e, exp, z, tile=tile) == (le(q), v), tile


# ------------------------------------------------------------------------------------- 3: open from evaluations
_BASIS = {}


def basis(gpu, tau_g1, exp):  # noqa: F811
    """The Lagrange basis over the golden powers, built once per exp."""
    if exp not in _BASIS:
        _BASIS[exp] = gpu.lagrange_basis(tau_g1, exp)
        assert _BASIS[exp] == gpu.g1_fft(tau_g1[: 96 << exp], exp).out
    return _BASIS[exp]


def witness_scalar(coeffs, z):
    return (poly_eval(coeffs, TAU) - poly_eval(coeffs, z)) * pow((TAU - z) % R, R - 2, R) % R


@pytest.mark.parametrize("exp,tile", [(0, 0), (1, 0), (5, 0), (10, 8)])
def test_open_evals(gpu, g1, powers, tau_g1, exp, tile):  # noqa: F811
    n, w = 1 << exp, omega(exp)
    c, e = polynomial(exp, seed=3)
    lag = basis(gpu, tau_g1, exp)
    commitment = gpu.kzg_commit_evals(lag, e)
    assert commitment == gpu.kzg_commit(powers, c) == g1([poly_eval(c, TAU)])
    table = gpu.open_domain_table(tau_g1[: 96 << exp], exp)
    all_proofs = gpu.kzg_open_domain(table, c, exp)
    ms = sorted({0, 1 % n, n - 1, 255 % n, 256 % n})
    for z, m in [(random.Random(80 + exp).randrange(R), None)] + [(pow(w, m, R), m) for m in ms]:
        proof = gpu.kzg_open_evals(lag, e, exp, z, tile=tile)
        ws = witness_scalar(c, z)
        assert proof.random_v is None and proof.value == poly_eval(c, z)
        assert proof.w == g1([ws])
        by_coeffs = gpu.kzg_open(powers, c, z)
        assert proof.w + le([proof.value]) == by_coeffs.w + le([by_coeffs.value])
        if m is not None:
            assert proof.w == all_proofs.proofs[96 * m: 96 * m + 96] and proof.value == all_proofs.values[m]
        # the check equation in the exponent: C = [w (tau - z) + value] G
        assert commitment == g1([(ws * (TAU - z) + proof.value) % R])
    if exp == 0:
        assert proof.w == INF1


def test_open_evals_window_and_montgomery_bases(gpu, g1, tau_g1):  # noqa: F811
    exp = 5
    c, e = polynomial(exp, seed=4)
    lag = basis(gpu, tau_g1, exp)
    z = random.Random(91).getrandbits(256)
    want = gpu.g1_kzg_open_evals(lag, e, exp, z)
    assert (want.ret, want.first_bad) == (0, -1)
    assert want.out == g1([witness_scalar(c, z % R)]) + le([poly_eval(c, z % R)])
    for window, tile in ((3, 8), (5, 0), (16, 12)):
        assert gpu.g1_kzg_open_evals(lag, e, exp, z, window=window, tile=tile) == want
    mont = gpu.deserialize_unchecked(lag)
    assert mont.ret == 0 and len(mont.out) == 104 << exp
    assert gpu.g1_kzg_open_evals(mont.out, e, exp, z, mont=True) == want
    assert gpu.g1_kzg_open_evals(mont.out, e, exp, z, mont=True, window=7) == want


def test_open_evals_malformed_basis_records(gpu, tau_g1):  # noqa: F811
    """x >= p at index 5 of 16, both SWFlags at index 2: the loaders' statuses, the smallest index, and
    `out` untouched."""
    import ctypes
    from kzgpot import _lib

    exp = 4
    lag = basis(gpu, tau_g1, exp)
    e = le(polynomial(exp, seed=5)[1])
    z = (99).to_bytes(32, "little")
    big = bytearray(lag)
    big[5 * 96: 5 * 96 + 48] = (O.P + 5).to_bytes(48, "little")
    flags = bytearray(lag)
    flags[2 * 96 + 95] |= 0xC0
    both = bytearray(big)
    both[2 * 96 + 95] |= 0xC0
    for data, want in ((big, (-3, 5)), (flags, (-6, 2)), (both, (-6, 2))):
        r = gpu.g1_kzg_open_evals(bytes(data), e, exp, 99)
        assert (r.ret, r.first_bad, r.out) == (*want, b"")
        out = ctypes.create_string_buffer(b"\xab" * 128, 128)
        fb = ctypes.c_int64(-1)
        assert _lib.load().kzgpot_g1_kzg_open_evals(bytes(data), e, exp, z, out, 0, ctypes.byref(fb)) == want[0]
        assert fb.value == want[1] and out.raw == b"\xab" * 128
        with pytest.raises(gpu.KzgPotError) as err:
            gpu.kzg_open_evals(bytes(data), e, exp, 99)
        assert (err.value.code, err.value.first_bad) == want
    with pytest.raises(gpu.KzgPotError) as err:
        bad = bytearray(tau_g1[: 96 * 16])
        bad[7 * 96: 7 * 96 + 48] = O.P.to_bytes(48, "little")
        gpu.lagrange_basis(bytes(bad), exp)
    assert (err.value.code, err.value.first_bad) == (-3, 7)


# ------------------------------------------------------------------------------------- 4: device entries, side stream
def test_dev_on_a_side_stream(gpu, tau_g1):  # noqa: F811
    import torch
    from kzgpot import device as D

    dev = torch.device("cuda:0")
    to_dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    exp = 9
    n = 1 << exp
    c, e = polynomial(exp)
    lag = basis(gpu, tau_g1, exp)
    z = pow(omega(exp), 300, R)  # on the domain: all four kernels of the division run
    want = gpu.g1_kzg_open_evals(lag, e, exp, z)
    assert want.ret == 0
    d_lag, d_e = to_dev(lag), to_dev(le(e))
    out = torch.full((128,), 0xAB, dtype=torch.uint8, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work = D.g1_kzg_open_evals_dev(d_lag, d_e, exp, z, out, key)
    side.synchronize()
    assert work.numel() == gpu.kzg_open_evals_workspace(exp)
    assert D.read_key(key) == (1 << 64) - 1
    assert bytes(out.cpu().numpy()) == want.out

    bad = d_lag.clone()
    bad[96 * 33: 96 * 33 + 48] = to_dev((O.P + 1).to_bytes(48, "little"))
    out.fill_(0xAB)
    with torch.cuda.stream(side):
        D.g1_kzg_open_evals_dev(bad, d_e, exp, z, out, key, work=work)
    side.synchronize()
    assert D.read_key(key) == (33 << 8) | 3
    assert bytes(out.cpu().numpy()) == b"\xab" * 128

    # the division's own device entry, evaluate-only included
    q, v = reference(c, exp, z)
    d_q = torch.full((32 * n + 32,), 0xAB, dtype=torch.uint8, device=dev)
    d_v = torch.full((64,), 0xAB, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(side):
        work = D.fr_evals_divide_dev(d_e, exp, z, d_q, d_v[:32], tile=8)
        D.fr_evals_divide_dev(d_e, exp, z, None, d_v[32:], tile=8, work=work)
    side.synchronize()
    assert work.numel() == gpu.fr_evals_workspace(exp, 8 << 16)
    assert bytes(d_q.cpu().numpy()) == le(q) + b"\xab" * 32
    assert bytes(d_v.cpu().numpy()) == le([v, v])
