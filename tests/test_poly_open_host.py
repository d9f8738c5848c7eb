"""Host-side parts of the polynomial division and KZG10 open: the workspace sizes, the argument
checks that are decided before any device use (so they hold without a GPU), and a model of the
tiled reverse scan of csrc/poly_kernels.hip — the document of its schedule, as test_msm_model.py
is for the MSM.

The model runs the kernels' own steps (a lane's Horner over its run of M = S / 256 entries, the
tree over the 256 run sums, the carry from the level above into lane 255, the 8-step suffix scan,
Horner from the lane's carry) on whole levels at once with numpy, over the prime 2^31 - 1 instead
of r: the schedule does not depend on the field, and products of two residues fit an int64. Its
power table is the kernels' (z^(2^k), level k reads entries k t + j)."""
import ctypes

import numpy as np
import pytest

E_INVALID_ARG = -100
MAX_N = (1 << 26) + 1
P = (1 << 31) - 1


# ------------------------------------------------------------------------------------- sizes
def test_workspaces_reject_invalid_flags_and_tiles(kzgpot_mod):
    k = kzgpot_mod
    for tile in (1, 7, 13, 15):
        assert k.fr_poly_workspace(1000, tile << 16) == 0
        assert k.kzg_open_workspace(1000, 3, tile << 16) == 0
    for flags in (1, 1 << 8, 1 << 15, 1 << 20, 1 << 31):  # the MSM's flags are not the division's
        assert k.fr_poly_workspace(1000, flags) == 0
    for flags in (2, 1 << 13, 1 << 20, 1 << 31, 17 << 8):  # unknown bits; a window width above 16
        assert k.kzg_open_workspace(1000, 3, flags) == 0
    assert k.fr_poly_workspace(MAX_N) > 0 and k.fr_poly_workspace(MAX_N + 1) == 0
    assert k.kzg_open_workspace(MAX_N, 0) > 0
    assert k.kzg_open_workspace(MAX_N + 1, 0) == 0 and k.kzg_open_workspace(5, MAX_N + 1) == 0
    assert k.kzg_open_workspace(MAX_N, 2) == 0  # 2^26 + 1 bases: above the MSM's limit
    for tile in (0, 8, 9, 10, 11, 12):
        assert k.fr_poly_workspace(0, tile << 16) >= 256
        assert k.kzg_open_workspace(0, 0, tile << 16 | 1 | 12 << 8) > 0


def test_workspaces_are_monotone_in_n(kzgpot_mod):
    k = kzgpot_mod
    ns = [0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 65536, 65537, 1 << 20, (1 << 20) + 1, 1 << 22,
          (1 << 24) + 1, 1 << 26, MAX_N]
    for tile in (0, 8, 12):
        sizes = [k.fr_poly_workspace(n, tile << 16) for n in ns]
        assert all(s >= 256 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), tile
        # the levels above the coefficients: one 32-byte entry per tile of the level below
        assert sizes[-1] >= 32 * -(-MAX_N >> (tile or 11))
    for nb in (0, 3, 1024):
        sizes = [k.kzg_open_workspace(n, nb) for n in ns if n - 1 + nb - 1 <= 1 << 26]
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), nb
    sizes = [k.kzg_open_workspace(1 << 16, nb) for nb in ns[:14]]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    # the staged bases, the quotients and the MSM's own workspace are all inside
    n = 1 << 16
    assert k.kzg_open_workspace(n, 0) >= (n - 1) * (96 + 32) + k.msm_workspace(False, n - 1) + k.fr_poly_workspace(n)
    assert k.kzg_open_workspace(n, 0, 1) >= (n - 1) * (104 + 32) + k.msm_workspace(False, n - 1, 1)


# ------------------------------------------------------------------------------------- argument errors
def test_argument_errors_need_no_gpu(kzgpot_mod):
    from kzgpot import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(4096)
    z = ctypes.create_string_buffer(32)
    fb = ctypes.c_int64(0)
    div, div_dev = lib.kzgpot_fr_poly_divide, lib.kzgpot_fr_poly_divide_dev
    for bad in (dict(coeffs=None), dict(z=None), dict(value=None), dict(flags=1), dict(flags=1 << 20),
                dict(flags=7 << 16), dict(flags=13 << 16), dict(n=MAX_N + 1)):
        a = dict(coeffs=buf, n=4, z=z, quotient=buf, value=buf, flags=0)
        a.update(bad)
        assert div(a["coeffs"], a["n"], a["z"], a["quotient"], a["value"], a["flags"]) == E_INVALID_ARG, bad
        assert div_dev(a["coeffs"], a["n"], a["z"], a["quotient"], a["value"], a["flags"], buf, None) == E_INVALID_ARG, bad
    assert div_dev(buf, 4, z, buf, buf, 0, None, None) == E_INVALID_ARG  # no workspace

    opn, opn_dev = lib.kzgpot_g1_kzg_open, lib.kzgpot_g1_kzg_open_dev
    for bad in (dict(pg=None), dict(coeffs=None), dict(pgg=None), dict(blind=None), dict(z=None), dict(out=None),
                dict(flags=2), dict(flags=1 << 13), dict(flags=1 << 20), dict(flags=17 << 8), dict(flags=5 << 16),
                dict(flags=13 << 16), dict(n=MAX_N + 1), dict(nb=MAX_N + 1), dict(n=MAX_N, nb=2), dict(n=1 << 26, nb=3)):
        a = dict(pg=buf, coeffs=buf, n=4, pgg=buf, blind=buf, nb=3, z=z, out=buf, flags=0)
        a.update(bad)
        args = (a["pg"], a["coeffs"], a["n"], a["pgg"], a["blind"], a["nb"], a["z"], a["out"], a["flags"])
        assert opn(*args, ctypes.byref(fb)) == E_INVALID_ARG, bad
        assert opn_dev(*args, buf, buf, None) == E_INVALID_ARG, bad
    args = (buf, buf, 4, buf, buf, 3, z, buf, 0)
    assert opn_dev(*args, None, buf, None) == E_INVALID_ARG  # no workspace
    assert opn_dev(*args, buf, None, None) == E_INVALID_ARG  # no key


def test_python_wrappers_check_before_the_library(kzgpot_mod):
    k = kzgpot_mod
    powers = k.Powers(np.zeros((7, 104), np.uint8), np.zeros((4, 104), np.uint8))
    with pytest.raises(ValueError):
        k.kzg_open(powers, [1] * 8, 5)
    with pytest.raises(ValueError):
        k.kzg_open(powers, [1] * 7, 5, blinding=[1] * 5)
    with pytest.raises(ValueError):
        k.fr_poly_divide(bytes(33), 5)
    with pytest.raises(ValueError):
        k.poly_flags(16)
    with pytest.raises(k.KzgPotError) as err:
        k.fr_poly_divide([1, 2, 3], 5, tile=7)
    assert err.value.code == E_INVALID_ARG


# ------------------------------------------------------------------------------------- the schedule's model
def horner_suffix(c, z):
    """H[j] = sum_{k >= j} c[k] z^(k - j), by the plain serial recurrence."""
    h, acc = [0] * len(c), 0
    for j in range(len(c) - 1, -1, -1):
        acc = (acc * z + int(c[j])) % P
        h[j] = acc
    return h


class Model:
    def __init__(self, z, t):
        self.t, self.S, self.M = t, 1 << t, 1 << (t - 8)
        self.zp = [z % P]
        for _ in range(63):
            self.zp.append(self.zp[-1] * self.zp[-1] % P)

    def tiles(self, a):
        """the level as (tiles, 256 lanes, M entries), zero past its end"""
        nt = -(-len(a) // self.S)
        pad = np.zeros(nt * self.S, np.int64)
        pad[: len(a)] = a
        return pad.reshape(nt, 256, self.M)

    def run_sums(self, x, y):
        acc = x[:, :, self.M - 1].copy()
        for i in range(self.M - 2, -1, -1):
            acc = (acc * y + x[:, :, i]) % P
        return acc

    def up(self, a, k):
        """one sum per tile: k_poly_up"""
        pw = self.zp[k * self.t:]
        acc = self.run_sums(self.tiles(a), pw[0])
        for s in range(8):  # a'[i] = a[2 i] + y a[2 i + 1]
            acc = (acc[:, 0::2] + pw[self.t - 8 + s] * acc[:, 1::2]) % P
        return acc[:, 0]

    def down(self, a, k, above):
        """the level's H from the H of the level above: k_poly_down"""
        pw = self.zp[k * self.t:]
        x = self.tiles(a)
        acc = self.run_sums(x, pw[0])
        carry = np.zeros(len(x), np.int64)
        if above is not None:
            assert len(above) == len(x)
            carry[:-1] = above[1:]
        acc[:, 255] = (acc[:, 255] + pw[self.t - 8] * carry) % P
        for s in range(8):  # suffix scan
            d = 1 << s
            acc[:, : 256 - d] = (acc[:, : 256 - d] + pw[self.t - 8 + s] * acc[:, d:]) % P
        h = np.concatenate([acc[:, 1:], carry[:, None]], axis=1)
        out = np.empty_like(x)
        for i in range(self.M - 1, -1, -1):
            h = (h * pw[0] + x[:, :, i]) % P
            out[:, :, i] = h
        return out.reshape(-1)[: len(a)]

    def divide(self, c):
        levels = [np.asarray(c, np.int64)]
        while len(levels[-1]) > self.S:
            levels.append(self.up(levels[-1], len(levels) - 1))
        h = None
        for k in range(len(levels) - 1, -1, -1):
            h = self.down(levels[k], k, h)
        return len(levels), h


def boundary_sizes(t):
    S = 1 << t
    ns = [1, 2, 255, 257, S - 1, S, S + 1, 2 * S + 3]
    for top in (S * S, S * S * S):
        if top <= 1 << 24:
            ns += [top, top + 1]
    return ns


@pytest.mark.parametrize("t", [8, 9, 10, 11, 12])
def test_model_of_the_tiled_scan_equals_horner(t):
    rng = np.random.default_rng(t)
    S = 1 << t
    for n in boundary_sizes(t):
        c = rng.integers(0, P, size=n, dtype=np.int64)
        z = int(rng.integers(2, P))
        levels, h = Model(z, t).divide(c)
        want_levels = 1 + (n > S) + (n > S * S) + (n > S * S * S)
        assert levels == want_levels, (t, n)
        # H is the one solution of H[n-1] = c[n-1], H[j] = c[j] + z H[j+1]
        assert h[-1] == c[-1], (t, n)
        assert np.array_equal(h[:-1], (c[:-1] + z * h[1:]) % P), (t, n)
        if n <= 3 * S + 3:
            assert h.tolist() == horner_suffix(c, z), (t, n)


def test_model_special_points():
    c = np.arange(1, 1001, dtype=np.int64)
    for z in (0, 1, P - 1):
        _, h = Model(z, 8).divide(c)
        assert h.tolist() == horner_suffix(c, z), z
