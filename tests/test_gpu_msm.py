"""G1 / G2 multi-scalar multiplication and the KZG10 commit on top of it, bit-exact.

Bases are [k_i]G with known k_i, so every expected record is ONE oracle scalar multiplication,
[sum_i s_i k_i mod r]G, independent of window width, bucket order or schedule:
  * G1 bases are the golden transcript's tauG1 section (k_j = tau^j; tau, alpha as
    test_gpu_lagrange.py obtains them) or come from the C oracle (oracle_g1_scalar_mul_encode);
  * G2 bases come from the Python oracle's g2_mul (about 14 ms each): at most 64 distinct, cached.
Scalars are 256-bit integers used as integers, so the expected scalar reduces s_i k_i mod r only
at the end."""
import os
import random

import pytest

from conftest import GOLDEN

import kzgpot_oracle as O
from test_gpu_lagrange import ALPHA, TAU, g1_points, g2_points, omega

pytestmark = pytest.mark.gpu

R = O.R_ORDER
N = 1024
NG1 = 2 * N - 1
INF1 = O.ark_g1_serialize(O.ARK_G1_ZERO)
INF2 = O.ark_g2_serialize(O.ARK_G2_ZERO)
TAU_POW = [pow(TAU, j, R) for j in range(NG1)]
G2_K = [pow(TAU, j, R) for j in range(64)]  # the 64 distinct G2 bases


def dot(scalars, ks):
    return sum(s * k for s, k in zip(scalars, ks)) % R


def rand256(rng, n):
    return [rng.getrandbits(256) for _ in range(n)]


@pytest.fixture(scope="module")
def transcript():
    with open(os.path.join(GOLDEN, "transcript_n1024.bin"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def tau_g1(gpu, transcript):
    """The decoded tauG1 section: 2047 ark records of [tau^j]G1."""
    r = gpu.g1_decompress(transcript[64: 64 + NG1 * 48])
    assert r.ret == 0
    return r.out


@pytest.fixture(scope="module")
def g2_bases():
    return g2_points(G2_K)


@pytest.fixture(scope="module")
def g1(oracle_lib):
    return lambda ks: g1_points(oracle_lib, ks)


def ok(r):
    assert (r.ret, r.first_bad) == (0, -1)
    return r.out


# ------------------------------------------------------------------------------------- 1: trivial sizes
def test_empty_and_single(gpu, g1, g2_bases):
    assert ok(gpu.g1_msm(b"", b"")) == INF1
    assert ok(gpu.g2_msm(b"", [])) == INF2
    p = g1([12345])
    assert ok(gpu.g1_msm(p, [1])) == p
    assert ok(gpu.g1_msm(p, [0])) == INF1
    assert ok(gpu.g1_msm(p, [R])) == INF1
    h = g2_bases[192: 384]
    assert ok(gpu.g2_msm(h, [1])) == h
    assert ok(gpu.g2_msm(h, [R])) == INF2


# ------------------------------------------------------------------------------------- 2: sizes around a wave and a block
@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 257, 1000, 2047])
def test_g1_random_scalars(gpu, g1, tau_g1, n):
    s = rand256(random.Random(n), n)
    assert ok(gpu.g1_msm(tau_g1[: 96 * n], s)) == g1([dot(s, TAU_POW)])


# ------------------------------------------------------------------------------------- 3: more than L entries in a bucket
def test_g1_tiled_random_and_all_equal(gpu, g1, tau_g1):
    """16,376 bases: several levels of the segmented sum; with all scalars equal every window's
    points share one bucket (2047 x 8 entries, far above the 64 a lane may sum)."""
    bases, ks = tau_g1 * 8, TAU_POW * 8
    rng = random.Random(33)
    s = rand256(rng, len(ks))
    assert ok(gpu.g1_msm(bases, s)) == g1([dot(s, ks)])
    one = rng.getrandbits(256)
    assert ok(gpu.g1_msm(bases, [one] * len(ks))) == g1([one * sum(ks) % R])


# ------------------------------------------------------------------------------------- 4: every window width path
def test_g1_window_override(gpu, g1, tau_g1):
    n = 300
    s = rand256(random.Random(4), n)
    want = g1([dot(s, TAU_POW)])
    for c in (0, 1, 2, 7, 8, 13, 16):
        assert ok(gpu.g1_msm(tau_g1[: 96 * n], s, window=c)) == want, c


# ------------------------------------------------------------------------------------- 5: exceptional additions
def test_g1_exceptional_additions(gpu, g1):
    G, mG = g1([1]), g1([R - 1])
    msm = lambda bases: ok(gpu.g1_msm(bases, [1] * (len(bases) // 96), window=8))  # noqa: E731
    assert msm(G + G) == g1([2])
    assert msm(G + mG) == INF1
    assert msm(G + mG + G) == G
    assert msm(INF1 + G + INF1 + INF1 + g1([5]) + INF1) == g1([6])
    assert msm(INF1 * 5) == INF1
    # the same with the library's width and a scalar that spreads over every window
    s = (1 << 256) - 1
    assert ok(gpu.g1_msm(G + G + mG, [s, s, s])) == g1([s % R])


# ------------------------------------------------------------------------------------- 6: integer semantics, top window
def test_g1_extreme_scalars(gpu, g1, tau_g1):
    s = [(1 << 256) - 1, R - 1, R + 1, 1 << 255, 0, R, 1]
    want = g1([dot(s, TAU_POW)])
    for c in (0, 5, 16):  # 256 = 51 * 5 + 1: a one-bit top window; 16: a full one
        assert ok(gpu.g1_msm(tau_g1[: 96 * len(s)], s, window=c)) == want, c
    assert ok(gpu.g1_msm(tau_g1[: 96 * len(s)], b"".join(x.to_bytes(32, "little") for x in s))) == want


# ------------------------------------------------------------------------------------- 7: G2
@pytest.mark.parametrize("n", [1, 2, 64, 130])
def test_g2_random_scalars(gpu, g2_bases, n):
    ks = (G2_K * 3)[:n]
    s = rand256(random.Random(700 + n), n)
    assert ok(gpu.g2_msm((g2_bases * 3)[: 192 * n], s)) == g2_points([dot(s, ks)])


def test_g2_exceptional_and_override(gpu, g2_bases):
    H, mH = g2_points([1]), g2_points([R - 1])
    assert ok(gpu.g2_msm(H + H, [1, 1], window=8)) == g2_points([2])
    assert ok(gpu.g2_msm(H + mH, [1, 1], window=8)) == INF2
    rng = random.Random(72)
    one = rng.getrandbits(256)
    ks = G2_K * 3
    assert ok(gpu.g2_msm(g2_bases * 3, [one] * len(ks))) == g2_points([one * sum(ks) % R])
    s = rand256(rng, 64)
    assert ok(gpu.g2_msm(g2_bases, s, window=3)) == g2_points([dot(s, G2_K)])


# ------------------------------------------------------------------------------------- 8: malformed bases
def test_malformed_bases(gpu, tau_g1, g2_bases):
    good = bytearray(tau_g1[: 96 * 16])
    big = bytearray(good)
    big[5 * 96: 5 * 96 + 48] = (O.P + 5).to_bytes(48, "little")
    flags = bytearray(good)
    flags[2 * 96 + 95] |= 0xC0
    both = bytearray(big)
    both[2 * 96 + 95] |= 0xC0
    s = rand256(random.Random(8), 16)
    for data, want in ((big, (-3, 5)), (flags, (-6, 2)), (both, (-6, 2))):
        ld = gpu.deserialize_unchecked(bytes(data))
        assert (ld.ret, ld.first_bad) == want
        r = gpu.g1_msm(bytes(data), s)
        assert (r.ret, r.first_bad) == want and r.out == b""
    data = bytearray(g2_bases[: 192 * 4])
    data[1 * 192 + 96: 1 * 192 + 144] = O.P.to_bytes(48, "little")  # y.c0 = p at index 1
    r = gpu.g2_msm(bytes(data), s[:4])
    ld = gpu.deserialize_unchecked(bytes(data), g2=True)
    assert (r.ret, r.first_bad) == (ld.ret, ld.first_bad) == (-3, 1) and r.out == b""


# ------------------------------------------------------------------------------------- 9: Montgomery bases
def test_montgomery_bases(gpu, tau_g1, g2_bases):
    rng = random.Random(9)
    x = tau_g1[: 96 * 40] + INF1 + tau_g1[96 * 40: 96 * 50]
    s = rand256(rng, 51)
    mont = gpu.deserialize_unchecked(x)
    assert mont.ret == 0 and len(mont.out) == 104 * 51 and mont.out[104 * 40 + 96] == 1  # the infinity record
    want = gpu.g1_msm(x, s)
    assert want.ret == 0 and gpu.g1_msm(mont.out, s, mont=True) == want
    bad = bytearray(mont.out)
    bad[7 * 104 + 48: 7 * 104 + 96] = O.P.to_bytes(48, "little")  # y = p at index 7
    r = gpu.g1_msm(bytes(bad), s, mont=True)
    assert (r.ret, r.first_bad, r.out) == (-3, 7, b"")
    x2 = g2_bases[: 192 * 20] + INF2
    m2 = gpu.deserialize_unchecked(x2, g2=True)
    assert m2.ret == 0
    want = gpu.g2_msm(x2, s[:21])
    assert want.ret == 0 and gpu.g2_msm(m2.out, s[:21], mont=True) == want


# ------------------------------------------------------------------------------------- 10: device entry, side stream
def test_dev_on_a_side_stream(gpu, tau_g1):
    import torch
    from kzgpot import device as D

    n = 500
    s = b"".join(v.to_bytes(32, "little") for v in rand256(random.Random(10), n))
    x = tau_g1[: 96 * n]
    want = gpu.g1_msm(x, s)
    dev = torch.device("cuda:0")
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    bases, scal = to_dev(x), to_dev(s)
    out = torch.full((96,), 0xAB, dtype=torch.uint8, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work = D.g1_msm_dev(bases, scal, out, key)
    side.synchronize()
    assert work.numel() == gpu.msm_workspace(False, n)
    assert D.read_key(key) == (1 << 64) - 1
    assert want.ret == 0 and bytes(out.cpu().numpy()) == want.out

    bad = bytearray(x)
    bad[7 * 96: 7 * 96 + 48] = O.P.to_bytes(48, "little")
    out.fill_(0xAB)
    D.g1_msm_dev(to_dev(bad), scal, out, key, work=work)
    torch.cuda.synchronize()
    assert D.read_key(key) == (7 << 8) | 3
    assert bytes(out.cpu().numpy()) == b"\xab" * 96


# ------------------------------------------------------------------------------------- 11: KZG10 commit
@pytest.fixture(scope="module")
def powers(gpu, transcript):
    """load_kzg_setup of the config-1 file: preprocess of the golden transcript, n_log2 = 10."""
    p, _ = gpu.load_kzg_setup_buffer(gpu.preprocess_buffer(transcript, 10), 10)
    return p


def poly_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def test_kzg_commit(gpu, g1, powers):
    rng = random.Random(11)
    p = [rng.randrange(R) for _ in range(20)]  # degree 19
    q = [rng.randrange(R) for _ in range(2)]   # degree-1 blinding polynomial
    want = g1([(poly_eval(p, TAU) + ALPHA * poly_eval(q, TAU)) % R])
    assert gpu.kzg_commit(powers, p, q) == want
    assert gpu.kzg_commit(powers, p + [0, 0, R], q + [0]) == want  # trailing zeros (mod r) are dropped
    assert gpu.kzg_commit(powers, p) == g1([poly_eval(p, TAU)])
    assert gpu.kzg_commit(powers, []) == INF1
    with pytest.raises(ValueError):
        gpu.kzg_commit(powers, [1] * (NG1 + 1))
    with pytest.raises(ValueError):
        gpu.kzg_commit(powers, p, [1] * (N + 1))


# ------------------------------------------------------------------------------------- 12: Lagrange commit
def test_lagrange_commit_equals_monomial_commit(gpu, powers, tau_g1):
    """Commit to evaluations over the Lagrange basis from the group FFT = commit to the
    interpolating polynomial's coefficients over the monomial powers."""
    exp, rng = 6, random.Random(12)
    m, wi = 1 << exp, pow(omega(exp), R - 2, R)
    evals = [rng.randrange(R) for _ in range(m)]
    minv = pow(m, R - 2, R)
    coeffs = [minv * sum(e * pow(wi, i * j, R) for j, e in enumerate(evals)) % R for i in range(m)]  # inverse NTT
    lag = gpu.g1_fft(tau_g1[: 96 << exp], exp)
    assert lag.ret == 0
    assert ok(gpu.g1_msm(lag.out, evals)) == gpu.kzg_commit(powers, coeffs)
