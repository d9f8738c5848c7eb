"""Integer model of the multi-scalar multiplication's schedule (csrc/msm_kernels.hip)
and the two host-only entry points.

The model runs the kernel's steps — count, exclusive scan, scatter, K levels of chunked segment
sums, the bit partials as chunked sums over the static lists, the final double-and-add — on the
discrete logs k_i of the bases instead of the bases (P_i = [k_i]G, arithmetic mod r, 0 = the point
at infinity), so the result must be sum_i s_i k_i mod r with the scalars used as 256-bit integers.
It also reports the largest number of entries any lane sums, which the kernel's L bounds whatever
the scalars are."""
import bisect
import ctypes
import random

import pytest

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
L = 64  # csrc/plans.hpp kMsmChunk
MAX_N = 1 << 26


def exscan(cnt):
    off, run = [], 0
    for v in cnt:
        off.append(run)
        run += v
    return off + [run]


def msm_model(ks, scalars, c, level_outputs=None):
    """-> (sum_i s_i k_i mod r as the schedule computes it, the most entries one lane summed).
    level_outputs (a list, optional) receives the number of partial sums each bucket level wrote
    (tests/test_plan_units.py holds them against the lane counts of the C++ plan)."""
    n, nwin, mask = len(ks), -(-256 // c), (1 << c) - 1
    nb = nwin << c
    buckets = [(i, (j << c) | ((s >> (j * c)) & mask)) for i, s in enumerate(scalars) for j in range(nwin)
               if ks[i] % R and (s >> (j * c)) & mask]
    # count, scan, scatter (cursor counting down, as k_msm_scatter)
    cnt = [0] * nb
    for _, b in buckets:
        cnt[b] += 1
    off = exscan(cnt)
    entries = [None] * off[nb]
    for i, b in buckets:
        cnt[b] -= 1
        entries[off[b] + cnt[b]] = ks[i]
    assert not any(cnt) and None not in entries
    # K levels: bucket b's entries in chunks of L, one lane per chunk
    levels, reach, most = 1, L, 0
    while reach < n:
        reach *= L
        levels += 1
    for _ in range(levels):
        off_out = exscan([-(-(off[b + 1] - off[b]) // L) for b in range(nb)])
        out = []
        for q in range(off_out[nb]):
            b = bisect.bisect_right(off_out, q) - 1
            start = off[b] + (q - off_out[b]) * L
            end = min(start + L, off[b + 1])
            most = max(most, end - start)
            out.append(sum(entries[start:end]) % R)
        # the regions are sized by min(in, in / L + NB)
        assert len(out) <= min(len(entries), len(entries) // L + nb)
        if level_outputs is not None:
            level_outputs.append(len(out))
        entries, off = out, off_out
    assert all(off[b + 1] - off[b] <= 1 for b in range(nb))
    # bit partials: segment (j, bit) lists the buckets (j, d) with that bit of d set, entry e <-> d
    # by deleting the bit; chunks of L entries per lane, level after level (kept sparse here)
    seg_len, part = 1 << (c - 1), {}
    for bk in range(nb):
        if off[bk + 1] == off[bk]:
            continue
        j, d = bk >> c, bk & mask
        for bit in range(c):
            if d >> bit & 1:
                e = ((d >> (bit + 1)) << bit) | (d & ((1 << bit) - 1))
                assert e < seg_len and ((e >> bit) << (bit + 1)) | (1 << bit) | (e & ((1 << bit) - 1)) == d
                key = (j * c + bit, e // L)
                part[key] = (part.get(key, 0) + entries[off[bk]]) % R
    most = max(most, min(L, seg_len))
    seg_len = -(-seg_len // L)
    while seg_len > 1:
        nxt = {}
        for (seg, e), v in part.items():
            nxt[(seg, e // L)] = (nxt.get((seg, e // L), 0) + v) % R
        part, seg_len = nxt, -(-seg_len // L)
    assert all(e == 0 for _, e in part)
    # final ladder over the W c bit positions
    acc = 0
    for k in reversed(range(nwin * c)):
        acc = (2 * acc + part.get((k, 0), 0)) % R
    return acc, most


def expect(ks, scalars):
    return sum(s * k for s, k in zip(scalars, ks)) % R


def scalar_sets(rng, n):
    one = rng.getrandbits(256)
    special = [0, (1 << 256) - 1, R - 1, R]
    return {
        "random": [rng.getrandbits(256) for _ in range(n)],
        "equal": [one] * n,
        "special": [special[i % 4] for i in range(n)],
        "all ones": [(1 << 256) - 1] * n,
    }


@pytest.fixture(scope="module")
def lib(kzgpot_mod):
    from kzgpot import _lib
    return _lib.load()


@pytest.mark.parametrize("c", range(1, 17))
def test_every_width(c):
    """Partial top windows (256 mod c != 0) and full ones (c = 1, 2, 4, 8, 16)."""
    rng = random.Random(c)
    n = 70  # more than L, so the all-equal case needs a second level
    ks = [rng.randrange(R) for _ in range(n)]
    ks[3] = 0  # an infinite base
    for name, s in scalar_sets(rng, n).items():
        got, most = msm_model(ks, s, c)
        assert got == expect(ks, s), name
        assert most <= L


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000])
def test_chosen_width(lib, n):
    c = lib.kzgpot_msm_window_bits(n)
    assert 1 <= c <= 16
    rng = random.Random(n)
    ks = [rng.randrange(1, R) for _ in range(n)]
    for name, s in scalar_sets(rng, n).items():
        got, most = msm_model(ks, s, c)
        assert got == expect(ks, s), name
        assert most <= L, name
        if name == "equal" and n > L:
            assert most == L  # all n points of a window share one bucket: full chunks, never more


def model_cost(n, c):
    """include/kzgpot.h: n W + B + 43 (W max(min(n, 2^c), n / 64) + B / 64), integer arithmetic."""
    nwin = -(-256 // c)
    bits = (nwin * c) << (c - 1)
    return n * nwin + bits + 43 * (nwin * max(min(n, 1 << c), n // L) + bits // L)


def test_width_table_is_the_models_choice(lib):
    """Each threshold of the table is the smallest n at which the model prefers c to c - 1, and
    between thresholds the table is the model's best width among 8..16."""
    width = lambda n: lib.kzgpot_msm_window_bits(ctypes.c_uint64(n))  # noqa: E731
    assert width(0) == width(1) == 8
    for c in range(9, 17):
        lo, hi = 1, MAX_N
        while lo < hi:
            mid = (lo + hi) // 2
            if model_cost(mid, c) < model_cost(mid, c - 1):
                hi = mid
            else:
                lo = mid + 1
        assert (width(lo - 1), width(lo)) == (c - 1, c), (c, lo)
    rng = random.Random(5)
    for n in [rng.randrange(1, MAX_N + 1) for _ in range(2000)] + [1 << k for k in range(27)]:
        assert width(n) == min(range(8, 17), key=lambda c: (model_cost(n, c), c)), n


def test_window_bits_and_workspace(lib):
    ws = lambda g2, n, flags=0: lib.kzgpot_msm_workspace(g2, ctypes.c_uint64(n), flags)  # noqa: E731
    sizes = [0, 1, 2, 63, 64, 65, 1000, 4097, 1 << 16, (1 << 20) + 1, 1 << 22, 1 << 26]
    for n in sizes:
        assert 1 <= lib.kzgpot_msm_window_bits(ctypes.c_uint64(n)) <= 16
    assert 1 <= lib.kzgpot_msm_window_bits(ctypes.c_uint64((1 << 64) - 1)) <= 16
    for g2 in (0, 1):
        got = [ws(g2, n) for n in sizes]
        assert all(v > 0 for v in got) and got == sorted(got), got
        assert ws(g2, MAX_N + 1) == 0
        for c in range(1, 17):
            assert ws(g2, 1000, c << 8) > 0 and ws(g2, 1000, c << 8 | 1) > 0
        for c in range(17, 32):
            assert ws(g2, 1000, c << 8) == 0
        assert ws(g2, 1000, 0x2) == 0 and ws(g2, 1000, 1 << 13) == 0  # unknown flag bits
        assert ws(g2, 1 << 26, 1 << 8) == 0  # 2^26 x 256 windows: entries past 32 bits
    assert ws(1, 1000) > ws(0, 1000)
    # monotone across the thresholds of the width table too (the index array shrinks there)
    for t in (28416, 55872, 120384, 3669568):
        dense = [ws(0, n) for n in range(t - 300, t + 300, 7)]
        assert dense == sorted(dense), t
