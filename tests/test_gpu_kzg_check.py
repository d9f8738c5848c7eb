"""KZG10 check and batch_check on the GPU, as the reference's end_to_end_test_kzg ends: commit -> open ->
check -> batch_check, then every way a proof can be wrong.

The setup is synthetic with known trapdoors: powers_of_g[j] = [tau^j]G and powers_of_gamma_g[j] =
[gamma tau^j]G for a degree bound of 32, the verifier key (G, [gamma]G, H, [tau]H), all from oracle
scalar multiplications. The end-to-end tests make their proofs with the library's own kzg_commit and
kzg_open; the larger batches take theirs from the trapdoor,
    w = [ (p(tau) - p(z)) / (tau - z) + gamma (b(tau) - b(z)) / (tau - z) ] G,
one C-oracle scalar multiplication per point. What is compared is the verdict."""
import random

import numpy as np
import pytest

import kzgpot_oracle as O
from test_gpu_lagrange import g1_points, g2_points

pytestmark = pytest.mark.gpu

P, R = O.P, O.R_ORDER
TOP = (1 << 256) - 1
DEGREE = 32
TAU, GAMMA = (random.Random(0xC4EC).randrange(1, R) for _ in range(2))
TAU_POW = [pow(TAU, j, R) for j in range(DEGREE + 1)]


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


@pytest.fixture(scope="module")
def g1(oracle_lib):
    return lambda ks: g1_points(oracle_lib, ks)


@pytest.fixture(scope="module")
def setup(gpu, g1):
    """(Powers, VerifierKey, the key's 576 packed bytes, the ark records of powers_of_g)"""
    rows = lambda ark, g2: np.frombuffer(gpu.deserialize_unchecked(ark, g2=g2).out,  # noqa: E731
                                         dtype=np.uint8).reshape(-1, 200 if g2 else 104)
    pg_ark = g1(TAU_POW)
    powers = gpu.Powers(rows(pg_ark, False), rows(g1([GAMMA * t % R for t in TAU_POW]), False))
    vk_ark = g1([1, GAMMA]) + g2_points([1, TAU])
    v1, v2 = rows(vk_ark[:192], False), rows(vk_ark[192:], True)
    vk = gpu.VerifierKey(v1[0].tobytes(), v1[1].tobytes(), v2[0].tobytes(), v2[1].tobytes())
    return powers, vk, vk_ark, pg_ark


def test_verifier_key_records(gpu, setup):
    _, vk, vk_ark, _ = setup
    assert gpu.verifier_key_records(vk) == vk_ark and len(vk_ark) == gpu.VK_BYTES


# ------------------------------------------------------------------------------------- end to end, as the reference's test
@pytest.mark.parametrize("seed,hiding", [(1, True), (2, True), (3, False)])
def test_end_to_end(gpu, setup, seed, hiding):
    """end_to_end_test_kzg: ten polynomials of degree 2 .. 19, hiding with a degree-1 blinding polynomial;
    each is committed, opened and checked, then all ten go through one batch_check"""
    powers, vk, vk_ark, _ = setup
    rng = random.Random(seed)
    comms, points, values, proofs = [], [], [], []
    for _ in range(10):
        p = [rng.randrange(R) for _ in range(rng.randrange(2, 20) + 1)]
        b = [rng.randrange(R) for _ in range(2)] if hiding else None
        z = rng.randrange(R)
        c = gpu.kzg_commit(powers, p, b)
        proof = gpu.kzg_open(powers, p, z, blinding=b)
        assert proof.value == poly_eval(p, z) and (proof.random_v is not None) == hiding
        assert gpu.kzg_check(vk, c, z, proof.value, proof) is True
        comms.append(c), points.append(z), values.append(proof.value), proofs.append(proof)
    assert gpu.kzg_batch_check(vk, comms, points, values, proofs) is True  # randomizers drawn as ark draws them
    assert gpu.kzg_batch_check(vk_ark, b"".join(comms), points, values, proofs, randomizers=[1] + [rng.getrandbits(128) for _ in range(9)]) is True
    values[7] = (values[7] + 1) % R
    assert gpu.kzg_batch_check(vk, comms, points, values, proofs) is False


def test_end_to_end_with_a_loaded_key(gpu):
    """the loaders' own Powers and VerifierKey (the golden transcript's setup), rows as load_kzg_setup leaves them"""
    import os
    from conftest import GOLDEN

    with open(os.path.join(GOLDEN, "transcript_n1024.bin"), "rb") as f:
        powers, vk = gpu.load_kzg_setup_buffer(gpu.preprocess_buffer(f.read(), 10), 10)
    rng = random.Random(4)
    p, b, z = [rng.randrange(R) for _ in range(12)], [rng.randrange(R) for _ in range(2)], rng.randrange(R)
    c, proof = gpu.kzg_commit(powers, p, b), gpu.kzg_open(powers, p, z, blinding=b)
    assert gpu.kzg_check(vk, c, z, proof.value, proof) is True
    assert gpu.kzg_check(vk, c, z, proof.value + 1, proof) is False


# ------------------------------------------------------------------------------------- rejection
def test_check_rejects_each_change_alone(gpu, setup, g1):
    powers, vk, vk_ark, _ = setup
    rng = random.Random(5)
    p, b, z = [rng.randrange(R) for _ in range(9)], [rng.randrange(R) for _ in range(2)], rng.randrange(R)
    c, proof = gpu.kzg_commit(powers, p, b), gpu.kzg_open(powers, p, z, blinding=b)
    v, rv, w = proof.value, proof.random_v, proof.w
    assert gpu.kzg_check(vk_ark, c, z, v, w, random_v=rv) is True
    assert gpu.kzg_check(vk_ark, c, z + R, v + R, w, random_v=rv + R) is True  # any 256-bit integer, reduced
    assert gpu.kzg_check(vk_ark, c, z, (v + 1) % R, w, random_v=rv) is False
    assert gpu.kzg_check(vk_ark, c, (z + 1) % R, v, w, random_v=rv) is False
    assert gpu.kzg_check(vk_ark, c, z, v, w, random_v=(rv + 1) % R) is False
    assert gpu.kzg_check(vk_ark, c, z, v, w) is False  # a hiding proof taken as not hiding
    w2 = gpu.g1_msm(w, [2]).out
    assert gpu.kzg_check(vk_ark, c, z, v, w2, random_v=rv) is False
    other = gpu.kzg_commit(powers, [rng.randrange(R) for _ in range(9)], b)
    assert gpu.kzg_check(vk_ark, other, z, v, w, random_v=rv) is False
    two_h = g2_points([2])
    assert gpu.kzg_check(vk_ark[:384] + two_h, c, z, v, w, random_v=rv) is False
    # the trapdoor's own witness: the same bytes as the library's
    inv = pow((TAU - z) % R, R - 2, R)
    assert w == g1([((poly_eval(p, TAU) - v) + GAMMA * (poly_eval(b, TAU) - rv)) * inv % R])


# ------------------------------------------------------------------------------------- batches from the trapdoor
@pytest.fixture(scope="module")
def batch(g1):
    """300 honest openings (more than one 256-lane block of the Fr kernel), every third not hiding; points
    and randomizers include 2^256 - 1 and r + 5"""
    rng = random.Random(6)
    n = 300
    polys = [[rng.randrange(R) for _ in range(rng.randrange(1, 6))] for _ in range(n)]
    blinds = [[rng.randrange(R) for _ in range(2)] if i % 3 else [] for i in range(n)]
    points = [rng.getrandbits(256) for _ in range(n)]
    points[0], points[1], points[n - 1] = TOP, R + 5, TAU + 1
    rho = [1] + [rng.getrandbits(128) for _ in range(n - 1)]
    rho[1], rho[2], rho[n - 1] = TOP, R + 5, rng.getrandbits(256)
    values = [poly_eval(p, z % R) for p, z in zip(polys, points)]
    random_vs = [poly_eval(b, z % R) for b, z in zip(blinds, points)]
    comm_k, wit_k = [], []
    for p, b, z, v, rv in zip(polys, blinds, points, values, random_vs):
        inv = pow((TAU - z) % R, R - 2, R)
        comm_k.append((poly_eval(p, TAU) + GAMMA * poly_eval(b, TAU)) % R)
        wit_k.append(((poly_eval(p, TAU) - v) + GAMMA * (poly_eval(b, TAU) - rv)) * inv % R)
    comms, wits = g1(comm_k), g1(wit_k)
    return {"n": n, "comms": comms, "wits": wits, "points": points, "values": values, "random_vs": random_vs, "rho": rho}


def run_batch(gpu, vk, bt, n, values=None, rho=None, hiding=True, **kw):
    res = gpu.g1_kzg_batch_check(vk, bt["comms"][: 96 * n], bt["points"][:n], (values or bt["values"])[:n], bt["wits"][: 96 * n],
                                 bt["random_vs"][:n] if hiding else None, (rho or bt["rho"])[:n], **kw)
    assert res.ret in (0, 1) and res.first_bad == -1
    return res.ret == 1


@pytest.mark.parametrize("n", [1, 2, 10, 300])
def test_batch_sizes(gpu, setup, batch, n):
    vk = setup[2]
    assert run_batch(gpu, vk, batch, n) is True
    for i in sorted({0, n // 2, n - 1}):  # exactly one value changed: the first, a middle one, the last
        values = list(batch["values"])
        values[i] = (values[i] + 1) % R
        assert run_batch(gpu, vk, batch, n, values=values) is False, i
    if n == 300:
        assert run_batch(gpu, vk, batch, n, window=5) is True
        assert run_batch(gpu, vk, batch, n, hiding=False) is False  # the random_vs dropped


def test_batch_beyond_256_share_blocks(gpu, setup, batch):
    """n = 65,700: 257 blocks leave 257 shares of each sum, so k_check_sums' sum_entries takes a second
    pass (shares 256 ...). The 300 honest openings 219 times over with fresh distinct randomizers; one
    value changed at 0, at 65,535 / 65,536 (the last entry of block 255, the first of block 256: the last
    share of the first pass and the first of the second) and at n - 1; several; one random_v in block 256."""
    vk, t = setup[2], 219
    n = 300 * t
    assert n == 65700 and (n + 255) // 256 == 257
    rng = random.Random(10)
    rho = [1] + [rng.getrandbits(128) for _ in range(n - 1)]
    rho[65535], rho[65536] = TOP, R + 5
    assert len(set(rho)) == n
    le = lambda vs: b"".join(v.to_bytes(32, "little") for v in vs)  # noqa: E731
    comms, wits, points, rho = batch["comms"] * t, batch["wits"] * t, le(batch["points"]) * t, le(rho)
    values, random_vs = batch["values"] * t, batch["random_vs"] * t

    def run(values=values, random_vs=random_vs):
        res = gpu.g1_kzg_batch_check(vk, comms, points, le(values), wits, le(random_vs), rho)
        assert res.ret in (0, 1) and res.first_bad == -1
        return res.ret == 1

    def changed(vs, *at):
        vs = list(vs)
        for i in at:
            vs[i] = (vs[i] + 1) % R
        return vs

    assert run() is True
    for i in (0, 65535, 65536, n - 1):
        assert run(values=changed(values, i)) is False, i
    assert run(values=changed(values, 7, 40000, 65536, 65650)) is False
    assert 65600 // 256 == 256 and batch["random_vs"][65600 % 300] != 0
    assert run(random_vs=changed(random_vs, 65600)) is False
    # none hiding: the non-hiding third alone, 657 times over, without random_vs
    plain = [i for i in range(300) if not batch["random_vs"][i] and i % 3 == 0]
    assert len(plain) == 100
    pick = lambda recs: b"".join(recs[96 * i: 96 * i + 96] for i in plain) * 657  # noqa: E731
    pvalues = [batch["values"][i] for i in plain] * 657
    ppoints = le([batch["points"][i] for i in plain]) * 657
    res = gpu.g1_kzg_batch_check(vk, pick(batch["comms"]), ppoints, le(pvalues), pick(batch["wits"]), None, rho)
    assert (res.ret, res.first_bad) == (1, -1)
    res = gpu.g1_kzg_batch_check(vk, pick(batch["comms"]), ppoints, le(changed(pvalues, 65536)), pick(batch["wits"]), None, rho)
    assert (res.ret, res.first_bad) == (0, -1)


def test_check_of_two_infinities(gpu, setup):
    """C = W = infinity: both pairs of the product are skipped; accepted for the value 0 at any point, and
    only for it"""
    vk = setup[2]
    inf = O.ark_g1_serialize(O.ARK_G1_ZERO)
    for z in (0, 1, TAU, TOP):
        assert gpu.kzg_check(vk, inf, z, 0, inf) is True
        assert gpu.kzg_check(vk, inf, z, R, inf) is True
        assert gpu.kzg_check(vk, inf, z, 1, inf) is False
    assert gpu.kzg_check(vk, inf, 5, 0, inf, random_v=1) is False


def test_batch_empty(gpu, setup):
    assert gpu.kzg_batch_check(setup[2], [], [], [], []) is True
    assert gpu.g1_kzg_batch_check(setup[2], b"", b"", b"", b"", None, b"").ret == 1


def test_randomizers_catch_the_classic_forgery(gpu, setup, g1):
    """Two honest proofs at one point z, the claimed values off by +d and -d: with the randomizers (1, 1)
    the errors cancel in sum rho_i v_i and the batch is accepted (why ark draws them); any other rho_1
    rejects it"""
    vk = setup[2]
    rng = random.Random(7)
    z, d = rng.randrange(R), rng.randrange(1, R)
    polys = [[rng.randrange(R) for _ in range(5)] for _ in range(2)]
    inv = pow((TAU - z) % R, R - 2, R)
    comms = g1([poly_eval(p, TAU) for p in polys])
    wits = g1([(poly_eval(p, TAU) - poly_eval(p, z)) * inv % R for p in polys])
    honest = [poly_eval(p, z) for p in polys]
    forged = [(honest[0] + d) % R, (honest[1] - d) % R]
    check = lambda values, rho: gpu.kzg_batch_check(vk, comms, [z, z], values, [wits[:96], wits[96:]], randomizers=rho)  # noqa: E731
    assert check(honest, [1, 1]) is True
    assert check(forged, [1, 1]) is True
    assert check(forged, [1, rng.getrandbits(128)]) is False
    assert check(honest, [1, rng.getrandbits(128)]) is True
    assert gpu.kzg_check(vk, comms[:96], z, forged[0], wits[:96]) is False  # each alone is plainly wrong


# ------------------------------------------------------------------------------------- the other openers
def test_open_domain_proofs_pass_one_batch(gpu, setup):
    vk, pg_ark = setup[2], setup[3]
    exp, n = 4, 16
    rng = random.Random(8)
    p = [rng.randrange(R) for _ in range(n)]
    c = gpu.kzg_commit(setup[0], p)
    dom = gpu.kzg_open_domain(gpu.open_domain_table(pg_ark, exp), p, exp)
    w = gpu.fr_domain_root(exp)
    points = [pow(w, i, R) for i in range(n)]
    rho = [1] + [rng.getrandbits(128) for _ in range(n - 1)]
    proofs = [dom.proofs[96 * i: 96 * i + 96] for i in range(n)]
    assert gpu.kzg_batch_check(vk, [c] * n, points, dom.values, proofs, randomizers=rho) is True
    shifted = dom.values[1:] + dom.values[:1]
    assert gpu.kzg_batch_check(vk, [c] * n, points, shifted, proofs, randomizers=rho) is False


def test_open_evals_proof_passes_check(gpu, setup):
    vk, pg_ark = setup[2], setup[3]
    exp = 4
    rng = random.Random(9)
    evals = [rng.randrange(R) for _ in range(1 << exp)]
    lag = gpu.lagrange_basis(pg_ark, exp)
    c = gpu.kzg_commit_evals(lag, evals)
    for z in (rng.randrange(R), pow(gpu.fr_domain_root(exp), 5, R)):  # off the domain, on it
        proof = gpu.kzg_open_evals(lag, evals, exp, z)
        assert gpu.kzg_check(vk, c, z, proof.value, proof) is True
        assert gpu.kzg_check(vk, c, z, (proof.value + 1) % R, proof) is False


# ------------------------------------------------------------------------------------- malformed records
def test_malformed_records(gpu, setup, batch):
    vk = setup[2]
    n = 10
    over = (P + 5).to_bytes(48, "little")

    def run(comms=None, wits=None, key=None):
        return gpu.g1_kzg_batch_check(key or vk, comms or batch["comms"][: 96 * n], batch["points"][:n], batch["values"][:n],
                                      wits or batch["wits"][: 96 * n], batch["random_vs"][:n], batch["rho"][:n])

    def patched(data, at, new):
        b = bytearray(data)
        b[at: at + len(new)] = new
        return bytes(b)

    def flagged(data, last):
        b = bytearray(data)
        b[last] |= 0xC0
        return bytes(b)

    comms, wits = batch["comms"][: 96 * n], batch["wits"][: 96 * n]
    r = run(comms=patched(comms, 4 * 96, over))
    assert (r.ret, r.first_bad) == (-3, 4)
    r = run(wits=patched(wits, 7 * 96 + 48, over))
    assert (r.ret, r.first_bad) == (-3, n + 7)
    r = run(comms=flagged(comms, 9 * 96 + 95), wits=patched(wits, 0, over))
    assert (r.ret, r.first_bad) == (-6, 9)  # the smallest index along commitments, proofs, vk
    r = run(wits=flagged(wits, 2 * 96 + 95))
    assert (r.ret, r.first_bad) == (-6, n + 2)
    # the four records of the key: g, gamma_g, h, beta_h
    for i, (at, status) in enumerate([(0, 3), (96 + 48, 3), (192 + 48, 3), (384 + 96, 3)]):
        r = run(key=patched(vk, at, over))
        assert (r.ret, r.first_bad) == (-status, 2 * n + i), i
    for i, last in enumerate([95, 191, 383, 575]):
        r = run(key=flagged(vk, last))
        assert (r.ret, r.first_bad) == (-6, 2 * n + i), i
    r = run(wits=patched(wits, 3 * 96, over), key=flagged(vk, 575))
    assert (r.ret, r.first_bad) == (-3, n + 3)
    with pytest.raises(gpu.KzgPotError) as err:
        gpu.kzg_batch_check(patched(vk, 192, over), [comms[:96]], [1], [1], [wits[:96]], randomizers=[1])
    assert (err.value.code, err.value.first_bad) == (-3, 2 + 2)
    with pytest.raises(gpu.KzgPotError) as err:
        gpu.kzg_check(vk, comms[:96], 1, 1, flagged(wits[:96], 95))
    assert (err.value.code, err.value.first_bad) == (-6, 1)
    assert run().ret == 1  # nothing is left behind


# ------------------------------------------------------------------------------------- device entry, side stream
def test_dev_on_a_side_stream(gpu, setup, batch):
    import torch
    from kzgpot import device as D

    n = 40
    le = lambda vs: b"".join(v.to_bytes(32, "little") for v in vs)  # noqa: E731
    dev = torch.device("cuda:0")
    to_dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)  # noqa: E731
    d_vk, d_c, d_w = to_dev(setup[2]), to_dev(batch["comms"][: 96 * n]), to_dev(batch["wits"][: 96 * n])
    d_z, d_v = to_dev(le(batch["points"][:n])), to_dev(le(batch["values"][:n]))
    d_rv, d_rho = to_dev(le(batch["random_vs"][:n])), to_dev(le(batch["rho"][:n]))
    out = torch.full((D.GT_OUT_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work = D.kzg_batch_check_dev(d_vk, d_c, d_z, d_v, d_w, d_rho, out, key, d_random_vs=d_rv)
    side.synchronize()
    assert work.numel() == gpu.kzg_batch_check_workspace(n)
    assert D.read_key(key) == (1 << 64) - 1
    got = bytes(out.cpu().numpy())
    assert got[:576] == (1).to_bytes(48, "little") + bytes(528) and got[576:] == (1).to_bytes(4, "little")

    d_v2 = d_v.clone()
    d_v2[32 * 11] = d_v2[32 * 11] ^ 1
    D.kzg_batch_check_dev(d_vk, d_c, d_z, d_v2, d_w, d_rho, out, key, d_random_vs=d_rv, work=work)
    torch.cuda.synchronize()
    got = bytes(out.cpu().numpy())
    assert D.read_key(key) == (1 << 64) - 1 and got[576:] == bytes(4) and got[:576] != (1).to_bytes(48, "little") + bytes(528)

    bad = d_w.clone()
    bad[5 * 96: 5 * 96 + 48] = to_dev((P + 1).to_bytes(48, "little"))
    out.fill_(0xAB)
    D.kzg_batch_check_dev(d_vk, d_c, d_z, d_v, bad, d_rho, out, key, d_random_vs=d_rv, work=work)
    torch.cuda.synchronize()
    assert D.read_key(key) == ((n + 5) << 8) | 3
    assert bytes(out.cpu().numpy()) == b"\xab" * D.GT_OUT_BYTES
