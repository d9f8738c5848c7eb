"""The NTT over Fr (csrc/ntt_kernels.hip through kzgpot_fr_ntt / kzgpot_fr_ntt_dev) against Python
integers: the O(m^2) definition up to exp 6, an iterative integer NTT above (test_ntt_units.py holds
both and checks one against the other). Inputs are random 256-bit integers with the edge values
0, r - 1, r, r + 1, 2r + 1 and 2^256 - 1 at both ends."""
import ctypes

import pytest

import kzgpot
from test_ntt_units import EDGES, R, TILES, TOP, ntt_inputs, ntt_ref, omega

pytestmark = pytest.mark.gpu

T = kzgpot.NTT_DEFAULT_TILE  # the library's tile (test_default_tile checks it against the library)
SIZES = sorted({0, 1, 2, 7, 8, 9, T - 1, T, T + 1, 2 * T, 2 * T + 1})


def le(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def ints(data):
    return [int.from_bytes(data[o: o + 32], "little") for o in range(0, len(data), 32)]


_REF = {}


def case(exp):
    """(inputs, forward, inverse) for exp, computed once and shared."""
    if exp not in _REF:
        x = ntt_inputs(exp, 0xC0DE + exp)
        _REF[exp] = (x, ntt_ref(x, exp), ntt_ref(x, exp, inverse=True))
    return _REF[exp]


def test_default_tile(gpu):
    """T above is the tile the library chooses: 2^T elements are one pass (no staging array in the
    workspace), which a smaller tile is not."""
    ws = lambda t: gpu.fr_ntt_workspace(T, t << 16)  # noqa: E731
    assert ws(0) == ws(T) and (T == TILES[0] or ws(0) < ws(T - 1))
    if T < TILES[-1]:
        assert gpu.fr_ntt_workspace(T + 1, 0) > gpu.fr_ntt_workspace(T + 1, (T + 1) << 16)


@pytest.mark.parametrize("exp", [e for e in SIZES if e <= 17])
def test_forward_and_inverse(gpu, exp):
    x, fwd, inv = case(exp)
    if exp >= 4:
        assert x[:6] == EDGES and x[-6:] == EDGES
    assert ints(gpu.fr_ntt(x, exp)) == fwd
    assert ints(gpu.fr_ntt(le(x), exp, inverse=True)) == inv


def all_outputs_agree(x, out, base, scale, rho):
    """True iff out[i] = scale sum_j x[j] base^(ij) for EVERY i < m (base a primitive m-th root), in
    O(m) integer operations: both sides as polynomials in i's generating variable at the random
    point rho,
        sum_i out[i] rho^i  =  scale sum_j x[j] sum_i (base^j rho)^i  =  scale (rho^m - 1) sum_j x[j] / (base^j rho - 1).
    If any out[i] differs, the two sides are different polynomials of degree < m in rho and agree
    at no more than m of the r > 2^254 possible points. The m inverses are one batch inversion."""
    m = len(x)
    lhs = 0
    for v in reversed(out):
        lhs = (lhs * rho + v) % R
    den, bj = [0] * m, rho
    for j in range(m):
        den[j] = (bj - 1) % R
        bj = bj * base % R
    pre = [1] * (m + 1)
    for j in range(m):
        pre[j + 1] = pre[j] * den[j] % R
    assert pre[m]  # rho is on no coset that makes a denominator zero
    inv, acc = pow(pre[m], R - 2, R), 0
    for j in range(m - 1, -1, -1):
        acc = (acc + x[j] * (inv * pre[j] % R)) % R
        inv = inv * den[j] % R
    return lhs == scale * (pow(rho, m, R) - 1) % R * acc % R


@pytest.mark.parametrize("exp", [e for e in SIZES if e > 17])
def test_forward_and_inverse_large(gpu, exp):
    """2^2T and 2^(2T+1) elements: two full passes, and a third of one stage. The input is dense,
    random 256-bit integers with the edge values at both ends, so every block and butterfly works
    on live data. The iterative integer transform of this size takes Python 3 to 6 s per
    direction, so the outputs are compared with Python integers in two other ways: ALL of them
    through the identity of all_outputs_agree at a random point, and a handful (both ends, the
    middle, a random index) one by one with the definition, out[i] = p(w^i) by Horner."""
    import random

    m = 1 << exp
    rng = random.Random(exp)
    data = bytearray(rng.randbytes(32 * m))
    for k, v in enumerate(EDGES):
        data[32 * k: 32 * k + 32] = data[32 * (m - 6 + k): 32 * (m - 5 + k)] = v.to_bytes(32, "little")
    data = bytes(data)
    x = [v % R for v in ints(data)]
    w, minv = omega(exp), pow(m, R - 2, R)
    winv = pow(w, R - 2, R)
    fwd, inv = ints(gpu.fr_ntt(data, exp)), ints(gpu.fr_ntt(data, exp, inverse=True))
    assert max(fwd) < R and max(inv) < R
    rho = rng.randrange(2, R)
    assert all_outputs_agree(x, fwd, w, 1, rho)
    assert all_outputs_agree(x, inv, winv, minv, rho)

    def horner(z):
        acc = 0
        for c in reversed(x):
            acc = (acc * z + c) % R
        return acc

    for i in (1, m - 1):
        assert fwd[i] == horner(pow(w, i, R)), (exp, i)
    i = rng.randrange(m)
    assert fwd[i] == horner(pow(w, i, R)) and inv[i] == horner(pow(winv, i, R)) * minv % R, (exp, i)
    assert fwd[0] == sum(x) % R and inv[m >> 1] == horner(R - 1) * minv % R


def test_three_passes_at_tile_8(gpu):
    """exp 17 at tile 8: passes of 8, 8 and 1 stages."""
    x, fwd, inv = case(17)
    assert ints(gpu.fr_ntt(x, 17, tile=8)) == fwd
    assert ints(gpu.fr_ntt(x, 17, inverse=True, tile=8)) == inv


def test_result_does_not_depend_on_the_tile(gpu):
    x, fwd, inv = case(13)
    for t in TILES:
        assert ints(gpu.fr_ntt(x, 13, tile=t)) == fwd, t
        assert ints(gpu.fr_ntt(x, 13, inverse=True, tile=t)) == inv, t


@pytest.mark.parametrize("exp", [5, 12, 13])
def test_round_trip_and_delta(gpu, exp):
    x = case(exp)[0]
    assert ints(gpu.fr_ntt(gpu.fr_ntt(x, exp), exp, inverse=True)) == [v % R for v in x]
    delta = [0, 1] + [0] * ((1 << exp) - 2)
    w = omega(exp)
    assert ints(gpu.fr_ntt(delta, exp)) == [pow(w, i, R) for i in range(1 << exp)]


def test_dev_entry_in_place_and_side_stream(gpu):
    """One block, two passes and (tile 8) three passes, out of place and in place, on a side stream
    with one workspace reused by every call of a size."""
    import torch
    from kzgpot import device as D

    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    for exp, tile in ((9, 0), (13, 0), (17, 8)):
        x, fwd, inv = case(exp)
        d_x = torch.frombuffer(bytearray(le(x)), dtype=torch.uint8).to(dev)
        d_out = torch.full((32 << exp,), 0xAB, dtype=torch.uint8, device=dev)
        d_io, d_io2 = d_x.clone(), d_x.clone()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            work = D.fr_ntt_dev(d_x, exp, d_out, tile=tile)
            D.fr_ntt_dev(d_io, exp, d_io, tile=tile, work=work)
            D.fr_ntt_dev(d_io2, exp, d_io2, inverse=True, tile=tile, work=work)
        side.synchronize()
        assert work.numel() == gpu.fr_ntt_workspace(exp, tile << 16)
        assert bytes(d_x.cpu().numpy()) == le(x)  # the input of an out-of-place call is untouched
        assert ints(bytes(d_out.cpu().numpy())) == fwd
        assert bytes(d_io.cpu().numpy()) == bytes(d_out.cpu().numpy())
        assert ints(bytes(d_io2.cpu().numpy())) == inv


def test_invalid_arguments(gpu):
    """-100 before any device use: the output keeps its fill."""
    from kzgpot import _lib

    lib = _lib.load()
    x = le([1, 2, 3, 4])
    out = ctypes.create_string_buffer(b"\xab" * 128, 128)
    bad_flags = [2, 1 << 8, 7 << 16, 12 << 16, 1 << 20]
    import torch

    d = torch.full((128,), 0xAB, dtype=torch.uint8, device="cuda:0")  # real memory, should a check fail
    work = torch.empty(gpu.fr_ntt_workspace(2), dtype=torch.uint8, device="cuda:0")
    dev = lib.kzgpot_fr_ntt_dev
    for exp, flags in [(27, 0)] + [(2, f) for f in bad_flags]:
        assert lib.kzgpot_fr_ntt(x, exp, out, flags) == -100, (exp, flags)
        assert dev(d.data_ptr(), exp, d.data_ptr(), flags, work.data_ptr(), None) == -100, (exp, flags)
    assert lib.kzgpot_fr_ntt(None, 2, out, 0) == -100 and lib.kzgpot_fr_ntt(x, 2, None, 0) == -100
    assert dev(None, 2, d.data_ptr(), 0, work.data_ptr(), None) == -100
    assert dev(d.data_ptr(), 2, None, 0, work.data_ptr(), None) == -100
    assert dev(d.data_ptr(), 2, d.data_ptr(), 0, None, None) == -100
    torch.cuda.synchronize()
    assert bytes(d.cpu().numpy()) == b"\xab" * 128
    assert out.raw == b"\xab" * 128
    for exp, flags in [(27, 0)] + [(2, f) for f in bad_flags]:
        assert gpu.fr_ntt_workspace(exp, flags) == 0
    with pytest.raises(ValueError):
        gpu.fr_ntt(x, 3)
    with pytest.raises(ValueError):
        gpu.fr_ntt(x, 2, tile=12)
    assert TOP % R == ints(gpu.fr_ntt([TOP], 0))[0]
