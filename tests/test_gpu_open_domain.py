"""Amortized KZG10 openings over a domain (kzgpot_g1/g2_open_domain_table, kzgpot_g1/g2_open_domain;
DESIGN.md §12), bit-exact.

The setup is the golden transcript's ([tau^j]G1, [tau^j]G2 with the tau test_gpu_lagrange.py
obtains), so every expected point is ONE oracle scalar multiplication of the generator,
independent of any FFT schedule:
  * proofs[i] = [(p(tau) - p(w^i)) (tau - w^i)^-1]G, by a field inverse;
  * T[i] = [(tau^n - x^n) (tau - x)^-1]G with x = w_2n^i.
G1 points come from the C oracle, G2 points from the Python oracle (about 14 ms each: G2 stays at
exp <= 4)."""
import random

import pytest

import kzgpot_oracle as O
from test_gpu_lagrange import TAU, g1_points, g2_points, omega, tau_g1, tau_g2, transcript  # noqa: F401
from test_gpu_msm import poly_eval, powers  # noqa: F401
from test_ntt_units import ntt_ref

pytestmark = pytest.mark.gpu

R = O.R_ORDER
TOP = (1 << 256) - 1
INF1 = O.ark_g1_serialize(O.ARK_G1_ZERO)
INF2 = O.ark_g2_serialize(O.ARK_G2_ZERO)
assert (TAU - 1) % R and pow(TAU, 2048, R) != 1  # tau lies on none of the domains used here


def inv(a):
    return pow(a % R, R - 2, R)


def table_scalars(exp):
    n = 1 << exp
    tn = pow(TAU, n, R)
    xs = [pow(omega(exp + 1), i, R) for i in range(2 * n)]
    return [(tn - pow(x, n, R)) * inv(TAU - x) % R for x in xs]


def values_of(p, exp):
    p = [c % R for c in p]
    if exp <= 7:
        return [poly_eval(p, pow(omega(exp), i, R)) for i in range(1 << exp)]
    return ntt_ref(p + [0] * ((1 << exp) - len(p)), exp)


def proof_scalars(p, exp):
    pt, w = poly_eval([c % R for c in p], TAU), omega(exp)
    return [(pt - v) * inv(TAU - pow(w, i, R)) % R for i, v in enumerate(values_of(p, exp))]


_TABLES = {}


def g1_table(gpu, tau_g1, exp):
    """The table over the golden powers, built once per exp (checked by test_g1_table)."""
    if exp not in _TABLES:
        _TABLES[exp] = gpu.open_domain_table(tau_g1[: 96 << exp], exp)
    return _TABLES[exp]


@pytest.fixture(scope="module")
def g1(oracle_lib):
    return lambda ks: g1_points(oracle_lib, ks)


# ------------------------------------------------------------------------------------- G1
G1_EXPS = [0, 1, 2, 5, 6, 7, 10]  # 5 / 6 / 7: the 2n-point transform on both sides of the 64-butterfly switch


@pytest.mark.parametrize("exp", G1_EXPS)
def test_g1_table(gpu, g1, tau_g1, exp):
    assert g1_table(gpu, tau_g1, exp) == g1(table_scalars(exp))


@pytest.mark.parametrize("exp", G1_EXPS)
def test_g1_proofs_and_values(gpu, g1, tau_g1, exp):
    p = [random.Random(exp).randrange(R) for _ in range(1 << exp)]
    got = gpu.kzg_open_domain(g1_table(gpu, tau_g1, exp), p, exp)
    assert got.values == values_of(p, exp)
    assert got.proofs == g1(proof_scalars(p, exp))
    only = gpu.kzg_open_domain(g1_table(gpu, tau_g1, exp), p, exp, want_values=False)
    assert only.values is None and only.proofs == got.proofs


@pytest.mark.parametrize("nc", [0, 1, 2, 63, 64])
def test_g1_coefficient_counts(gpu, g1, tau_g1, nc):
    """Fewer coefficients than points: the missing ones are zero, so the scalars of the per-point
    pass are zero only by construction; none or one: every scalar is zero, every proof the point at
    infinity and every value c_0."""
    p = [random.Random(100 + nc).randrange(1, R) for _ in range(nc)]
    r = gpu.g1_open_domain(g1_table(gpu, tau_g1, 6), p, 6)
    assert (r.ret, r.first_bad) == (0, -1)
    proofs, values = r.out[: 96 * 64], r.out[96 * 64:]
    assert [int.from_bytes(values[o: o + 32], "little") for o in range(0, 2048, 32)] == values_of(p, 6)
    assert proofs == g1(proof_scalars(p, 6))
    if nc <= 1:
        assert proofs == INF1 * 64 and values == (p[0] if p else 0).to_bytes(32, "little") * 64


def test_g1_unreduced_tile_and_trailing_zeros(gpu, g1, tau_g1):
    table = g1_table(gpu, tau_g1, 6)
    rng = random.Random(7)
    p = [R, TOP, R + 1, 2 * R + 1] + [rng.getrandbits(256) for _ in range(40)]
    want = g1(proof_scalars(p, 6))
    for tile in (0, 8, 11):
        r = gpu.g1_open_domain(table, p, 6, tile=tile)
        assert r.ret == 0 and r.out[: 96 * 64] == want, tile
    assert gpu.g1_open_domain(table, p + [0] * 20, 6).out == r.out  # a zero tail as given
    assert gpu.kzg_open_domain(table, p + [0, R, 0], 6).proofs == want  # and trimmed


def test_g1_root_on_the_domain(gpu, g1, tau_g1):
    """p = (x - w^3) s(x): values[3] = 0 and proofs[3] = [s(tau)]G."""
    w3 = pow(omega(6), 3, R)
    s = [random.Random(9).randrange(R) for _ in range(63)]
    p = [((s[k - 1] if k else 0) - w3 * (s[k] if k < 63 else 0)) % R for k in range(64)]
    got = gpu.kzg_open_domain(g1_table(gpu, tau_g1, 6), p, 6)
    assert got.values[3] == 0 and got.values == values_of(p, 6)
    assert got.proofs[96 * 3: 96 * 4] == g1([poly_eval(s, TAU)])
    assert got.proofs == g1(proof_scalars(p, 6))


def test_g1_agrees_with_the_single_point_open(gpu, tau_g1, powers):  # noqa: F811
    """An extra consistency check, not the reference: kzg_open at w^i over the same setup."""
    p = [random.Random(12).randrange(R) for _ in range(64)]
    got = gpu.kzg_open_domain(g1_table(gpu, tau_g1, 6), p, 6)
    for i in (0, 1, 63):
        one = gpu.kzg_open(powers, p, pow(omega(6), i, R))
        assert one.w == got.proofs[96 * i: 96 * i + 96] and one.value == got.values[i]


# ------------------------------------------------------------------------------------- G2
@pytest.mark.parametrize("exp", [0, 2, 4])
def test_g2(gpu, tau_g2, exp):
    table = gpu.open_domain_table(tau_g2[: 192 << exp], exp, g2=True)
    assert table == g2_points(table_scalars(exp))
    p = [random.Random(20 + exp).randrange(R) for _ in range(1 << exp)]
    got = gpu.kzg_open_domain(table, p, exp, g2=True)
    assert got.values == values_of(p, exp)
    assert got.proofs == g2_points(proof_scalars(p, exp))
    if exp == 0:
        assert got.proofs == INF2


# ------------------------------------------------------------------------------------- malformed input
def test_malformed_records(gpu, tau_g1, tau_g2):
    table = bytearray(g1_table(gpu, tau_g1, 6))
    p = list(range(1, 65))
    bad = bytearray(table)
    bad[96 * 70: 96 * 70 + 48] = (O.P + 1).to_bytes(48, "little")  # x >= p
    bad[96 * 90 + 95] |= 0xC0  # both SWFlags, behind it
    r = gpu.g1_open_domain(bytes(bad), p, 6)
    assert (r.ret, r.first_bad, r.out) == (-3, 70, b"")
    bad = bytearray(table)
    bad[96 * 5 + 95] |= 0xC0
    r = gpu.g1_open_domain(bytes(bad), p, 6)
    assert (r.ret, r.first_bad, r.out) == (-6, 5, b"")
    # the table's own input: the index is the record's in `powers`, the smallest one
    pw = bytearray(tau_g1[: 96 * 64])
    pw[96 * 9: 96 * 9 + 48] = (O.P + 1).to_bytes(48, "little")
    pw[96 * 40 + 95] |= 0xC0
    with pytest.raises(gpu.KzgPotError) as e:
        gpu.open_domain_table(bytes(pw), 6)
    assert (e.value.code, e.value.first_bad) == (-3, 9)
    pw2 = bytearray(tau_g2[: 192 * 4])
    pw2[192 * 3 + 191] |= 0xC0
    with pytest.raises(gpu.KzgPotError) as e:
        gpu.open_domain_table(bytes(pw2), 2, g2=True)
    assert (e.value.code, e.value.first_bad) == (-6, 3)


def test_dev_on_a_side_stream_and_rejection_writes_nothing(gpu, g1, tau_g1):
    import torch
    from kzgpot import device as D

    dev = torch.device("cuda:0")
    to_dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    table = g1_table(gpu, tau_g1, 6)
    p = [random.Random(31).randrange(R) for _ in range(50)]
    d_table, d_p = to_dev(table), to_dev(b"".join(c.to_bytes(32, "little") for c in p))
    d_powers = to_dev(tau_g1[: 96 * 64])
    d_built = torch.full((2 * 96 * 64,), 0xAB, dtype=torch.uint8, device=dev)
    proofs = torch.full((96 * 64,), 0xAB, dtype=torch.uint8, device=dev)
    values = torch.full((32 * 64,), 0xAB, dtype=torch.uint8, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        D.open_domain_table_dev(False, d_powers, 6, d_built, key)
        work = D.g1_open_domain_dev(d_built, d_p, 6, proofs, values, key)
    side.synchronize()
    assert work.numel() == gpu.open_domain_workspace(False, 6)
    assert D.read_key(key) == (1 << 64) - 1
    assert bytes(d_built.cpu().numpy()) == table
    assert bytes(proofs.cpu().numpy()) == g1(proof_scalars(p, 6))
    assert [int.from_bytes(bytes(values[o: o + 32].cpu().numpy()), "little") for o in range(0, 2048, 32)] == values_of(p, 6)

    bad = d_table.clone()
    bad[96 * 33: 96 * 33 + 48] = to_dev((O.P + 1).to_bytes(48, "little"))
    proofs.fill_(0xAB)
    values.fill_(0xAB)
    with torch.cuda.stream(side):
        D.g1_open_domain_dev(bad, d_p, 6, proofs, values, key, work=work)
    side.synchronize()
    assert D.read_key(key) == (33 << 8) | 3
    assert bytes(proofs.cpu().numpy()) == b"\xab" * (96 * 64) and bytes(values.cpu().numpy()) == b"\xab" * (32 * 64)
    # the host entry leaves its outputs alone too
    import ctypes
    from kzgpot import _lib

    out_p, out_v = ctypes.create_string_buffer(b"\xab" * 6144, 6144), ctypes.create_string_buffer(b"\xab" * 2048, 2048)
    fb = ctypes.c_int64(-1)
    coeffs = bytes(d_p.cpu().numpy())
    assert _lib.load().kzgpot_g1_open_domain(bytes(bad.cpu().numpy()), coeffs, 50, 6, out_p, out_v, 0, ctypes.byref(fb)) == -3
    assert fb.value == 33 and out_p.raw == b"\xab" * 6144 and out_v.raw == b"\xab" * 2048


def test_invalid_arguments(gpu, tau_g1):
    import ctypes
    from kzgpot import _lib

    lib = _lib.load()
    table = g1_table(gpu, tau_g1, 2)
    with pytest.raises(ValueError):
        gpu.kzg_open_domain(table, [1, 2, 3, 4, 5], 2)  # n_coeffs = 2^exp + 1
    with pytest.raises(ValueError):
        gpu.kzg_open_domain(table, [1], 25)
    with pytest.raises(ValueError):
        gpu.open_domain_table(tau_g1, 25)
    with pytest.raises(ValueError):
        gpu.kzg_open_domain(table, [1, 2], 2, tile=12)
    out_p, out_v = ctypes.create_string_buffer(b"\xab" * 384, 384), ctypes.create_string_buffer(b"\xab" * 128, 128)
    fb = ctypes.c_int64(-1)
    c5 = b"".join(k.to_bytes(32, "little") for k in range(5))
    raw = lib.kzgpot_g1_open_domain
    assert raw(table, c5, 5, 2, out_p, out_v, 0, ctypes.byref(fb)) == -100
    assert raw(table, c5, 1, 25, out_p, out_v, 0, ctypes.byref(fb)) == -100
    assert raw(table, c5, 4, 2, out_p, out_v, 1, ctypes.byref(fb)) == -100  # KZGPOT_NTT_INVERSE is not the opening's
    assert raw(table, c5, 4, 2, out_p, out_v, 1 << 8, ctypes.byref(fb)) == -100
    assert raw(table, c5, 4, 2, out_p, out_v, 12 << 16, ctypes.byref(fb)) == -100
    assert raw(None, c5, 4, 2, out_p, out_v, 0, ctypes.byref(fb)) == -100
    assert raw(table, None, 4, 2, out_p, out_v, 0, ctypes.byref(fb)) == -100
    assert raw(table, c5, 4, 2, None, out_v, 0, ctypes.byref(fb)) == -100
    assert lib.kzgpot_g1_open_domain_table(None, 2, out_p, ctypes.byref(fb)) == -100
    assert lib.kzgpot_g2_open_domain_table(table, 25, out_p, ctypes.byref(fb)) == -100
    assert out_p.raw == b"\xab" * 384 and out_v.raw == b"\xab" * 128
    assert gpu.open_domain_workspace(False, 25) == 0 and gpu.open_domain_workspace(True, 4, 12 << 16) == 0
    assert gpu.open_domain_workspace(False, 4, 1) == 0 and gpu.open_domain_table_workspace(True, 25) == 0
    assert gpu.open_domain_workspace(True, 24) > gpu.open_domain_workspace(False, 24) > 0
    # values may be NULL: proofs only
    assert raw(table, c5, 4, 2, out_p, None, 0, ctypes.byref(fb)) == 0 and out_p.raw != b"\xab" * 384
