"""The product of pairings on the GPU against the pairing's definition (tests/pairing_model.py: affine
Miller loop in E(Fq12), the naive exponent d (p^12 - 1) / r). Every comparison is GT bytes or a boolean.
The many-pair products are built from three distinct model pairings repeated with known multiplicities,
so the CPU side is three pairings and a few Fq12 powers. The products with distinct data in every lane —
up to the cap of 2^16 pairs, with infinities by position, an inverse pair split across blocks and a reused
workspace — take bilinearity over the model's e(G1, G2) as their reference, itself checked once against
the definition. The kernels' functions below the whole call: tests/test_gpu_pairing_cells.py."""
import ctypes
import random

import pytest

import kzgpot_oracle as O
import pairing_model as M
from test_gpu_lagrange import g1_points

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


# ------------------------------------------------------------------------------------- distinct data per lane
# Bilinearity over the model's one pairing e = e(G1, G2): the product over ([a_i]G1, [b_i]G2) is
# e^(sum a_i b_i mod r) (d = 3 included, as e is). Every lane has a full-size a_i of its own (records from
# the C oracle) and one of 16 full-size b_i, so a lane that read a neighbour's word, or a tree partner
# taken from the wrong lane, changes the product.
NB = 16


def b_of(i):
    return (7 * i + i // NB) % NB  # never the neighbour's


@pytest.fixture(scope="module")
def lanes(oracle_lib, pairs):
    """(e, a_i, the G1 records of [a_i]G1, b_j, the G2 records of [b_j]G2) for 520 lanes"""
    rng = random.Random(0x1A9E5)
    a = [rng.randrange(1 << 254, R) for _ in range(520)]
    bs = [rng.randrange(1 << 254, R) for _ in range(NB)]
    assert len(set(a)) == len(a) and len(set(bs)) == NB and all(b_of(i) != b_of(i + 1) for i in range(70000))
    rec1 = g1_points(oracle_lib, a)
    return pairs[0][2], a, [rec1[96 * i: 96 * i + 96] for i in range(len(a))], bs, [g2(O.g2_mul(G2, b)) for b in bs]


def expect(e, exponent):
    exponent %= R
    return (exponent == 0, M.f12_to_bytes(M.f12_pow(e, exponent)))


def test_bilinear_reference_is_the_model(gpu, lanes, pairs):
    """the reference of the tests below, once against the definition: pairs[2] is a random pair"""
    e, a, rec1, bs, rec2 = lanes
    assert O.ark_g1_serialize((*O.g1_mul(G1, a[0]), False)) == rec1[0]
    assert gpu.pairing_product(rec1[0], rec2[3]) == (False, M.f12_to_bytes(M.pairing(O.g1_mul(G1, a[0]), O.g2_mul(G2, bs[3]))))
    assert gpu.pairing_product(rec1[0], rec2[3]) == expect(e, a[0] * bs[3])


@pytest.mark.parametrize("k", [64, 65, 256, 257, 513])
def test_products_of_distinct_pairs(gpu, lanes, k):
    e, a, rec1, bs, rec2 = lanes
    got = gpu.pairing_product(b"".join(rec1[:k]), b"".join(rec2[b_of(i)] for i in range(k)))
    assert got == expect(e, sum(a[i] * bs[b_of(i)] for i in range(k)))


def test_infinities_by_position(gpu, lanes):
    e, a, rec1, bs, rec2 = lanes
    k = 257
    inf1 = {0, 63, 64, 256, 200} | set(range(128, 192, 2)) | set(range(129, 192, 3))
    inf2 = {1, 65, 255, 200} | set(range(129, 192, 2)) | set(range(128, 192, 3))
    assert set(range(128, 192)) <= inf1 | inf2 and inf1 & inf2 >= {200, 128, 135}
    live = [i for i in range(k) if i not in inf1 | inf2]
    r1 = b"".join(g1(None) if i in inf1 else rec1[i] for i in range(k))
    r2 = b"".join(g2(None) if i in inf2 else rec2[b_of(i)] for i in range(k))
    assert gpu.pairing_product(r1, r2) == expect(e, sum(a[i] * bs[b_of(i)] for i in live))
    # every lane but one
    for only in (130, 256):
        r1 = b"".join(rec1[i] if i == only or i % 2 else g1(None) for i in range(k))
        r2 = b"".join(rec2[b_of(i)] if i == only or not i % 2 else g2(None) for i in range(k))
        assert gpu.pairing_product(r1, r2) == expect(e, a[only] * bs[b_of(only)])


def test_inverse_pair_split_across_blocks(gpu, lanes, oracle_lib):
    """(P, Q) at lane 3 and (-P, Q) at lane 300 among 320 live pairs: the product is the others' alone"""
    e, a, rec1, bs, rec2 = lanes
    k = 320
    neg = g1_points(oracle_lib, [R - a[3]])
    assert neg[:48] == rec1[3][:48] and neg != rec1[3]
    r1 = [rec1[i] for i in range(k)]
    r2 = [rec2[b_of(i)] for i in range(k)]
    r1[300], r2[300] = neg, r2[3]
    others = sum(a[i] * bs[b_of(i)] for i in range(k) if i not in (3, 300))
    got = gpu.pairing_product(b"".join(r1), b"".join(r2))
    assert got == expect(e, others) and got[0] is False


def test_workspace_reuse_on_the_device_entry(gpu, lanes):
    """one workspace sized for 257 pairs and filled with 0xFF runs k = 257, then 3, then 0: each result is the
    host call's; nothing relies on a zeroed or a fresh workspace"""
    import torch
    from kzgpot import device as D

    e, a, rec1, bs, rec2 = lanes
    dev = torch.device("cuda:0")
    to_dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev) if x else torch.empty(0, dtype=torch.uint8, device=dev)  # noqa: E731
    work = torch.full((gpu.pairing_workspace(257),), 0xFF, dtype=torch.uint8, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    for k in (257, 3, 0):
        r1, r2 = b"".join(rec1[:k]), b"".join(rec2[b_of(i)] for i in range(k))
        out = torch.full((D.GT_OUT_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
        assert D.pairing_product_dev(to_dev(r1), to_dev(r2), out, key, work=work) is work
        torch.cuda.synchronize()
        one, gt = gpu.pairing_product(r1, r2)
        assert D.read_key(key) == (1 << 64) - 1
        assert bytes(out.cpu().numpy()) == gt + int(one).to_bytes(4, "little"), k
        assert (one, gt) == expect(e, sum(a[i] * bs[b_of(i)] for i in range(k))), k


@pytest.mark.parametrize("k", [65536, 65281])
def test_products_at_the_cap(gpu, lanes, k):
    """the cap of 2^16 pairs, where the tree's second level is a full block of 256 values 256 lanes apart, and
    255 * 256 + 1, where its last value comes from a block of one. The records cycle through 299 distinct
    pairs: 299 is coprime to 64 and 256, so neighbours and tree partners differ."""
    import time

    e, a, rec1, bs, rec2 = lanes
    m = 299
    assert gpu.PAIRING_MAX_PAIRS == 65536 >= k and gpu.pairing_workspace(65537) == 0 and k in (65536, 255 * 256 + 1)
    r1 = (b"".join(rec1[:m]) * (k // m + 1))[: 96 * k]
    r2 = (b"".join(rec2[b_of(i)] for i in range(m)) * (k // m + 1))[: 192 * k]
    t0 = time.perf_counter()
    got = gpu.pairing_product(r1, r2)
    print(f"pairing_product, k = {k}: {time.perf_counter() - t0:.3f} s")
    assert got == expect(e, sum(a[i % m] * bs[b_of(i % m)] for i in range(k)))


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
