"""The product of pairings on the GPU against the pairing's definition (tests/pairing_model.py: affine
Miller loop in E(Fq12), the naive exponent d (p^12 - 1) / r). Every comparison is GT bytes or a boolean.
The many-pair products are built from three distinct model pairings repeated with known multiplicities,
so the CPU side is three pairings and a few Fq12 powers."""
import ctypes
import random

import pytest

import kzgpot_oracle as O
import pairing_model as M

pytestmark = pytest.mark.gpu

P, R = O.P, O.R_ORDER
G1, G2 = O.G1_GEN, O.G2_GEN
E_INVALID_ARG = -100


def g1(p):
    return O.ark_g1_serialize(O.ARK_G1_ZERO if p is None else (p[0], p[1], False))


def g2(q):
    return O.ark_g2_serialize(O.ARK_G2_ZERO if q is None else (q[0], q[1], False))


def neg1(p):
    return (p[0], -p[1] % P)


@pytest.fixture(scope="module")
def pairs():
    """three pairs of subgroup points with the model's pairing of each: (G1, G2), ([a]G1, [b]G2), random"""
    rng = random.Random(0x9A1)
    a, b = rng.randrange(1, 1 << 20), rng.randrange(1, 1 << 20)
    pts = [(G1, G2), (O.g1_mul(G1, a), O.g2_mul(G2, b)), (O.g1_mul(G1, rng.randrange(R)), O.g2_mul(G2, rng.randrange(R)))]
    es = [M.pairing(p, q) for p, q in pts]
    assert es[1] == M.f12_pow(es[0], a * b)  # the model agrees with itself
    return [(p, q, e) for (p, q), e in zip(pts, es)]


def product(gpu, items):
    return gpu.pairing_product(b"".join(g1(p) for p, _ in items), b"".join(g2(q) for _, q in items))


def test_gt_power_is_stated(gpu):
    assert gpu.PAIRING_GT_POWER == M.D == 3 and gpu.GT_BYTES == 576


@pytest.mark.parametrize("which", [0, 1, 2], ids=["generators", "multiples", "random"])
def test_single_pairing_bytes(gpu, pairs, which):
    p, q, e = pairs[which]
    assert product(gpu, [(p, q)]) == (False, M.f12_to_bytes(e))


@pytest.mark.parametrize("k", [2, 3, 65, 257])  # over a wave of the Miller kernel, over a block of the tree
def test_products(gpu, pairs, k):
    rng = random.Random(k)
    picks = [rng.randrange(3) for _ in range(k)]
    want = M.F12_ONE
    for i in range(3):
        want = M.f12_mul(want, M.f12_pow(pairs[i][2], picks.count(i)))
    ok, gt = product(gpu, [pairs[i][:2] for i in picks])
    assert (ok, gt) == (False, M.f12_to_bytes(want))


def test_infinity_and_empty(gpu, pairs):
    p, q, e = pairs[2]
    assert product(gpu, []) == (True, M.GT_ONE_BYTES)
    assert product(gpu, [(None, q)]) == (True, M.GT_ONE_BYTES)
    assert product(gpu, [(p, None)]) == (True, M.GT_ONE_BYTES)
    assert product(gpu, [(None, None)]) == (True, M.GT_ONE_BYTES)
    assert product(gpu, [(None, q), (p, q), (p, None)]) == (False, M.f12_to_bytes(e))
    # an infinity record's coordinates are not looked at beyond their range
    junk = bytearray(g1(p))
    junk[95] |= 0x40
    assert gpu.pairing_product(bytes(junk), g2(q)) == (True, M.GT_ONE_BYTES)


def test_inverse_pairs(gpu, pairs):
    p, q, e = pairs[1]
    assert product(gpu, [(p, q), (neg1(p), q)]) == (True, M.GT_ONE_BYTES)
    assert product(gpu, [(p, q), (p, (q[0], O.fp2_neg(q[1])))]) == (True, M.GT_ONE_BYTES)
    # one byte changed, the point still valid but another one: the infinity flag of -P
    recs = bytearray(g1(p) + g1(neg1(p)))
    recs[96 + 95] |= 0x40
    assert gpu.pairing_product(bytes(recs), g2(q) * 2) == (False, M.f12_to_bytes(e))
    # and another point of the subgroup in its place
    ok, gt = product(gpu, [(p, q), (neg1(O.g1_mul(p, 2)), q)])
    assert (ok, gt) == (False, M.f12_to_bytes(M.f12_conj(e)))  # e e^-2 = e^-1, the conjugate in GT


def test_check_equation_of_two_pairings(gpu):
    """e([a]G1, [b]G2) e(-[a b]G1, G2) = 1"""
    a, b = 0x1234567, 0x7654321
    assert product(gpu, [(O.g1_mul(G1, a), O.g2_mul(G2, b)), (neg1(O.g1_mul(G1, a * b % R)), G2)])[0] is True
    assert product(gpu, [(O.g1_mul(G1, a), O.g2_mul(G2, b)), (neg1(O.g1_mul(G1, (a * b + 1) % R)), G2)])[0] is False


# ------------------------------------------------------------------------------------- malformed records
def c_product(gpu, g1_recs, g2_recs, k):
    from kzgpot import _lib

    out = ctypes.create_string_buffer(b"\xab" * 576, 576)
    fb = ctypes.c_int64(-7)
    ret = _lib.load().kzgpot_pairing_product(g1_recs, g2_recs, k, out, ctypes.byref(fb))
    return ret, fb.value, out.raw


def test_malformed_records(gpu, pairs):
    k = 5
    good1, good2 = g1(pairs[1][0]) * k, g2(pairs[1][1]) * k
    untouched = b"\xab" * 576
    over = (P + 3).to_bytes(48, "little")

    def with_bytes(recs, at, data):
        b = bytearray(recs)
        b[at: at + len(data)] = data
        return bytes(b)

    def with_flags(recs, rec, i):
        b = bytearray(recs)
        b[rec * i + rec - 1] |= 0xC0
        return bytes(b)

    # a coordinate >= p: x or y of g1[3]; x.c1 of g2[2], y.c0 of g2[4]
    assert c_product(gpu, with_bytes(good1, 3 * 96, over), good2, k) == (-3, 3, untouched)
    assert c_product(gpu, with_bytes(good1, 3 * 96 + 48, P.to_bytes(48, "little")), good2, k) == (-3, 3, untouched)
    assert c_product(gpu, good1, with_bytes(good2, 2 * 192 + 48, over), k) == (-3, k + 2, untouched)
    assert c_product(gpu, good1, with_bytes(good2, 4 * 192 + 96, over), k) == (-3, k + 4, untouched)
    # both flags set
    assert c_product(gpu, with_flags(good1, 96, 1), good2, k) == (-6, 1, untouched)
    assert c_product(gpu, good1, with_flags(good2, 192, 0), k) == (-6, k, untouched)
    # the smallest index along g1 then g2, whatever the lanes' order
    assert c_product(gpu, with_flags(good1, 96, 4), with_bytes(good2, 0, over), k) == (-6, 4, untouched)
    assert c_product(gpu, with_bytes(with_flags(good1, 96, 4), 2 * 96, over), good2, k) == (-3, 2, untouched)
    with pytest.raises(gpu.KzgPotError) as err:
        gpu.pairing_product(good1, with_flags(good2, 192, 3))
    assert (err.value.code, err.value.first_bad) == (-6, k + 3)
    # the call before left nothing behind
    ret, fb, out = c_product(gpu, good1[:96], good2[:192], 1)
    assert (ret, fb, out) == (0, -1, M.f12_to_bytes(pairs[1][2]))


def test_argument_errors(gpu):
    from kzgpot import _lib

    lib = _lib.load()
    fb = ctypes.c_int64(-1)
    out = ctypes.create_string_buffer(b"\xab" * 576, 576)
    cap = gpu.PAIRING_MAX_PAIRS
    assert lib.kzgpot_pairing_product(g1(G1), g2(G2), cap + 1, out, ctypes.byref(fb)) == E_INVALID_ARG
    assert lib.kzgpot_pairing_product(None, g2(G2), 1, out, ctypes.byref(fb)) == E_INVALID_ARG
    assert lib.kzgpot_pairing_product(g1(G1), None, 1, out, ctypes.byref(fb)) == E_INVALID_ARG
    assert out.raw == b"\xab" * 576
    assert gpu.pairing_workspace(cap + 1) == 0 < gpu.pairing_workspace(0) <= gpu.pairing_workspace(1) <= gpu.pairing_workspace(cap)
    assert lib.kzgpot_pairing_product(g1(G1), g2(G2), 1, None, None) == 0  # no GT wanted, no index wanted: not one


# ------------------------------------------------------------------------------------- device entry, side stream
def test_dev_on_a_side_stream(gpu, pairs):
    import torch
    from kzgpot import device as D

    items = [pairs[0][:2], pairs[2][:2], (None, G2)]
    want = M.f12_to_bytes(M.f12_mul(pairs[0][2], pairs[2][2]))
    dev = torch.device("cuda:0")
    to_dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    d1, d2 = to_dev(b"".join(g1(p) for p, _ in items)), to_dev(b"".join(g2(q) for _, q in items))
    out = torch.full((D.GT_OUT_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work = D.pairing_product_dev(d1, d2, out, key)
    side.synchronize()
    assert work.numel() == gpu.pairing_workspace(3)
    assert D.read_key(key) == (1 << 64) - 1
    assert bytes(out.cpu().numpy()) == want + (0).to_bytes(4, "little")

    bad = d2.clone()
    bad[192: 192 + 48] = to_dev((P + 1).to_bytes(48, "little"))
    out.fill_(0xAB)
    D.pairing_product_dev(d1, bad, out, key, work=work)
    torch.cuda.synchronize()
    assert D.read_key(key) == ((3 + 1) << 8) | 3
    assert bytes(out.cpu().numpy()) == b"\xab" * D.GT_OUT_BYTES
