"""The host-buffer form of every keyed entry point, called through ctypes so that the caller's buffers
are in sight: a malformed record gives -(status) and its index and leaves every output byte as it was;
the same call with the record restored succeeds and gives what the Python wrapper gives. Then the
optional arguments and the G2 variants of the device-tensor wrappers that no other file reaches.

The shapes are the smallest with an interior record (4 records, or 2 per side where the call takes
pairs). The corruption is the other files': x = p + 1, status 3 (not in the field). The expected
indices are include/kzgpot.h's: along the input records, for the open along powers_of_g then
powers_of_gamma_g, for the pairing along g1 then g2, for the check along commitments, proofs, vk."""
import ctypes
import random
from dataclasses import dataclass

import pytest

import kzgpot_oracle as O
from test_gpu_lagrange import g1_points, g2_points

pytestmark = pytest.mark.gpu

P, R = O.P, O.R_ORDER
FILL = 0xA5
NOT_IN_FIELD = 3
TAU, GAMMA = (random.Random(0x51A6).randrange(1, R) for _ in range(2))


def le(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def corrupted(records, i):
    b = bytearray(records)
    b[96 * i: 96 * i + 48] = (P + 1).to_bytes(48, "little")
    return bytes(b)


@dataclass
class Case:
    fn: str
    records: bytes      # the G1 records one of which is corrupted
    bad_record: int
    first_bad: int      # the index the call reports for it
    args: object        # (records, out) -> the arguments before first_bad; out(n) makes an output buffer
    ret: int            # of the valid call
    want: bytes         # the valid call's outputs end to end, from the Python wrapper


@pytest.fixture(scope="module")
def cases(gpu, oracle_lib):
    rng = random.Random(0xF0E1)
    g1 = lambda ks: g1_points(oracle_lib, ks)  # noqa: E731
    pts = g1([3, 5, 7, 11])
    sc4 = [rng.randrange(R) for _ in range(4)]
    z = rng.randrange(R)
    out = {}

    out["g1_fft"] = Case("kzgpot_g1_fft", pts, 2, 2, lambda r, o: (r, 2, o(4 * 96), 1), 0, gpu.g1_fft(pts, 2).out)
    out["g1_msm"] = Case("kzgpot_g1_msm", pts, 1, 1, lambda r, o: (r, le(sc4), 4, o(96), 0), 0, gpu.g1_msm(pts, sc4).out)

    # p of 4 coefficients over powers_of_g[:3], a blinding polynomial of 2 over powers_of_gamma_g[:1]
    blind, pgg = [rng.randrange(R) for _ in range(2)], g1([13])
    out["g1_kzg_open"] = Case("kzgpot_g1_kzg_open", pts[: 3 * 96], 1, 1,
                              lambda r, o: (r, le(sc4), 4, pgg, le(blind), 2, le([z]), o(160), 0), 0,
                              gpu.g1_kzg_open(pts[: 3 * 96], sc4, pgg, blind, z).out)

    table = gpu.open_domain_table(pts, 2)
    out["g1_open_domain_table"] = Case("kzgpot_g1_open_domain_table", pts, 1, 1, lambda r, o: (r, 2, o(8 * 96)), 0, table)
    out["g1_open_domain"] = Case("kzgpot_g1_open_domain", table, 5, 5,
                                 lambda r, o: (r, le(sc4), 4, 2, o(4 * 96), o(4 * 32), 0), 0,
                                 gpu.g1_open_domain(table, sc4, 2).out)
    out["g1_kzg_open_evals"] = Case("kzgpot_g1_kzg_open_evals", pts, 2, 2,
                                    lambda r, o: (r, le(sc4), 2, le([z]), o(128), 0), 0,
                                    gpu.g1_kzg_open_evals(pts, sc4, 2, z).out)

    # e([6]G, [7]H) e([-42]G, H) = 1
    pair_g1, pair_g2 = g1([6, R - 42]), g2_points([7, 1])
    res = gpu.g1g2_pairing_product(pair_g1, pair_g2)
    out["pairing_product"] = Case("kzgpot_pairing_product", pair_g1, 1, 1, lambda r, o: (r, pair_g2, 2, o(576)), 1, res.out)
    assert res.ret == 1

    # two honest hiding openings from the trapdoor, as tests/test_gpu_kzg_check.py makes its batches
    polys = [[rng.randrange(R) for _ in range(3)] for _ in range(2)]
    blinds = [[rng.randrange(R) for _ in range(2)] for _ in range(2)]
    points, rho = [rng.getrandbits(256) for _ in range(2)], [1, rng.getrandbits(128)]
    values = [poly_eval(p, x % R) for p, x in zip(polys, points)]
    random_vs = [poly_eval(b, x % R) for b, x in zip(blinds, points)]
    comms = g1([(poly_eval(p, TAU) + GAMMA * poly_eval(b, TAU)) % R for p, b in zip(polys, blinds)])
    wits = g1([((poly_eval(p, TAU) - v) + GAMMA * (poly_eval(b, TAU) - rv)) * pow((TAU - x) % R, R - 2, R) % R
               for p, b, x, v, rv in zip(polys, blinds, points, values, random_vs)])
    vk = g1([1, GAMMA]) + g2_points([1, TAU])
    res = gpu.g1_kzg_batch_check(vk, comms, points, values, wits, random_vs, rho)
    out["kzg_batch_check"] = Case("kzgpot_kzg_batch_check", comms, 1, 1,
                                  lambda r, o: (vk, r, le(points), le(values), wits, le(random_vs), le(rho), 2, 0), 1, b"")
    assert res.ret == 1 and res.first_bad == -1
    return out


def run(case, records):
    from kzgpot import _lib

    outs = []

    def out(n):
        outs.append(ctypes.create_string_buffer(bytes([FILL]) * n, n))
        return outs[-1]

    fb = ctypes.c_int64(7)
    ret = getattr(_lib.load(), case.fn)(*case.args(records, out), ctypes.byref(fb))
    return ret, fb.value, b"".join(b.raw for b in outs)


NAMES = ["g1_fft", "g1_msm", "g1_kzg_open", "g1_open_domain_table", "g1_open_domain", "g1_kzg_open_evals",
         "pairing_product", "kzg_batch_check"]


@pytest.mark.parametrize("name", NAMES)
def test_rejection_writes_nothing_then_the_valid_call_succeeds(cases, name):
    case = cases[name]
    ret, first_bad, written = run(case, corrupted(case.records, case.bad_record))
    assert (ret, first_bad) == (-NOT_IN_FIELD, case.first_bad)
    assert written == bytes([FILL]) * len(written)
    ret, first_bad, written = run(case, case.records)
    assert (ret, first_bad) == (case.ret, -1)
    assert written == case.want


# ------------------------------------------------------------------------------------- optional arguments
def test_open_domain_without_coefficients_and_values(gpu, oracle_lib, cases):
    from kzgpot import _lib

    table = cases["g1_open_domain"].records
    proofs = ctypes.create_string_buffer(bytes([FILL]) * 384, 384)
    fb = ctypes.c_int64(7)
    assert _lib.load().kzgpot_g1_open_domain(table, None, 0, 2, proofs, None, 0, ctypes.byref(fb)) == 0
    assert fb.value == -1 and proofs.raw == g1_points(oracle_lib, [0] * 4)  # the zero polynomial: infinity records
    assert proofs.raw == gpu.g1_open_domain(table, b"", 2, want_values=False).out


def test_pairing_product_without_the_gt_bytes(cases):
    from kzgpot import _lib

    case = cases["pairing_product"]
    fb = ctypes.c_int64(7)
    g1, g2 = case.records, case.args(case.records, lambda n: None)[1]
    assert _lib.load().kzgpot_pairing_product(g1, g2, 2, None, ctypes.byref(fb)) == 1 and fb.value == -1
    assert _lib.load().kzgpot_pairing_product(g1[96:] + g1[:96], g2, 2, None, ctypes.byref(fb)) == 0 and fb.value == -1
    assert _lib.load().kzgpot_pairing_product(corrupted(g1, 1), g2, 2, None, ctypes.byref(fb)) == -NOT_IN_FIELD
    assert fb.value == 1


# ------------------------------------------------------------------------------------- G2 device-tensor wrappers
def test_g2_device_wrappers_agree_with_the_host_forms(gpu):
    import torch
    from kzgpot import device as D

    dev = torch.device("cuda:0")
    to_dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    host = lambda t: bytes(t.cpu().numpy())  # noqa: E731
    fresh = lambda n: torch.full((n,), FILL, dtype=torch.uint8, device=dev)  # noqa: E731
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    no_bad = (1 << 64) - 1
    pts, sc = g2_points([3, 5]), [random.Random(0x62).randrange(R) for _ in range(2)]

    d_sum = fresh(192)
    work = D.g2_msm_dev(to_dev(pts), to_dev(le(sc)), d_sum, key)
    torch.cuda.synchronize()
    assert work.numel() == gpu.msm_workspace(True, 2) and D.read_key(key) == no_bad
    assert host(d_sum) == gpu.g2_msm(pts, sc).out

    d_table = fresh(4 * 192)
    work = D.open_domain_table_dev(True, to_dev(pts), 1, d_table, key)
    torch.cuda.synchronize()
    assert work.numel() == gpu.open_domain_table_workspace(True, 1) and D.read_key(key) == no_bad
    table = gpu.open_domain_table(pts, 1, g2=True)
    assert host(d_table) == table

    d_proofs, d_values = fresh(2 * 192), fresh(2 * 32)
    work = D.g2_open_domain_dev(d_table, to_dev(le(sc)), 1, d_proofs, d_values, key)
    torch.cuda.synchronize()
    assert work.numel() == gpu.open_domain_workspace(True, 1) and D.read_key(key) == no_bad
    assert host(d_proofs) + host(d_values) == gpu.g2_open_domain(table, sc, 1).out
