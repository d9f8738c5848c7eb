"""Integer model of the multi-scalar multiplication's schedule (csrc/msm_kernels.hip)
and the two host-only entry points.

The model runs the kernel's steps — count, exclusive scan, scatter, K levels of chunked segment
sums, the bit partials as chunked sums over the static lists, the final double-and-add — on the
discrete logs k_i of the bases instead of the bases (P_i = [k_i]G, arithmetic mod r, 0 = the point
at infinity), so the result must be sum_i s_i k_i mod r with the scalars used as 256-bit integers.
It also reports the largest number of entries any lane sums, which the kernel's L bounds whatever
the scalars are. On request it counts, per stage, the additions that meet one of jac_madd's
exceptional branches, lists the bit partials T_k, and scatters in a given wave order: the crafted
cases of tests/msm_cases.py are held against that census here and run on the device by
tests/test_gpu_msm_stages.py."""
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


STAGES = ("bucket0", "bucket1", "bucket2", "bits0", "bits1", "bits2", "final")
KINDS = ("double", "cancel", "after_cancel", "skipped")


class Sum:
    """One lane's accumulator over discrete logs, as k_msm_sum's and k_msm_final's: an infinite entry
    (0) is skipped as slot_of skips it (kind `skipped`, counted where the model holds the entry: an
    infinite partial sum of the level before; the empty buckets of mode 2 are not listed); every other
    addition is counted in census[(stage, kind)] when it meets acc == entry (double: jac_madd's
    `same` branch), acc == -entry (cancel: Z3 = 0) or a zero accumulator that has added before
    (after_cancel: Z1 = 0 with non-zero X, Y)."""

    def __init__(self, census, stage):
        self.v, self.adds, self.census, self.stage = 0, 0, census, stage

    def hit(self, kind):
        if self.census is not None:
            self.census[self.stage, kind] = self.census.get((self.stage, kind), 0) + 1

    def add(self, e):
        if not e:
            self.hit("skipped")
            return
        if not self.v:
            if self.adds:
                self.hit("after_cancel")
        elif self.v == e:
            self.hit("double")
        elif self.v + e == R:
            self.hit("cancel")
        self.v = (self.v + e) % R
        self.adds += 1


def scatter(ks, digit, n, nwin, c, cnt, off, order):
    """k_msm_scatter's bucket order. order None: the points in index order, each taking the slot
    below its bucket's cursor. order (kind, seed): wave by wave — a wave is 64 consecutive indices
    of a 256-lane block, lanes i >= n included; kind "index" takes the waves of every window in
    index order, "reversed" in reverse, "shuffle" in an order drawn from seed. A wave whose 64 lanes
    target one bucket takes 64 contiguous slots, lane l at old - 1 - l; any other wave's lanes take
    single slots, in index order or ("shuffle") in an order drawn from seed."""
    entries = [None] * off[-1]
    if order is None:
        for i in range(n):
            for j in range(nwin):
                b = digit(i, j)
                if b is not None:
                    cnt[b] -= 1
                    entries[off[b] + cnt[b]] = ks[i]
        return entries
    kind, seed = order
    rng = random.Random(seed)
    nwaves = max(1, -(-n // 256)) * 4
    for j in range(nwin):
        waves = list(range(nwaves))
        if kind == "reversed":
            waves.reverse()
        elif kind == "shuffle":
            rng.shuffle(waves)
        else:
            assert kind == "index"
        for w in waves:
            lanes = [(i, digit(i, j) if i < n else None) for i in range(64 * w, 64 * w + 64)]
            lead = lanes[0][1]
            if all(b == lead for _, b in lanes):
                if lead is None:
                    continue
                old = cnt[lead]
                assert old >= 64
                cnt[lead] -= 64
                for lane, (i, _) in enumerate(lanes):
                    entries[off[lead] + old - 1 - lane] = ks[i]
                continue
            if kind == "shuffle":
                rng.shuffle(lanes)
            for i, b in lanes:
                if b is not None:
                    cnt[b] -= 1
                    entries[off[b] + cnt[b]] = ks[i]
    return entries


def msm_model(ks, scalars, c, level_outputs=None, census=None, partials=None, order=None):
    """-> (sum_i s_i k_i mod r as the schedule computes it, the most entries one lane summed).
    level_outputs (a list, optional) receives the number of partial sums each bucket level wrote
    (tests/test_plan_units.py holds them against the lane counts of the C++ plan).
    census (a dict, optional) receives {(stage, kind): count} over STAGES x KINDS (class Sum), the
    bucket and bit levels past the third counted with the third.
    partials (a list, optional) receives the W c bit partials T_k as discrete logs, 0 = infinity.
    order (optional): the scatter's order inside a bucket (scatter above)."""
    n, nwin, mask = len(ks), -(-256 // c), (1 << c) - 1
    nb = nwin << c
    ks = [k % R for k in ks]
    used = -(-max(scalars, default=0).bit_length() // c)  # the windows above hold zero digits only

    def digit(i, j):  # the bucket of (point i, window j), as msm_bucket
        d = (scalars[i] >> (j * c)) & mask if j < used else 0
        return (j << c) | d if d and ks[i] else None

    # count, scan, scatter (cursor counting down, as k_msm_scatter)
    cnt = [0] * nb
    for i in range(n):
        for j in range(used):
            b = digit(i, j)
            if b is not None:
                cnt[b] += 1
    off = exscan(cnt)
    entries = scatter(ks, digit, n, used, c, cnt, off, order)
    assert not any(cnt) and None not in entries
    # K levels: bucket b's entries in chunks of L, one lane per chunk
    levels, reach, most = 1, L, 0
    while reach < n:
        reach *= L
        levels += 1
    for level in range(levels):
        off_out = exscan([-(-(off[b + 1] - off[b]) // L) for b in range(nb)])
        out = []
        for q in range(off_out[nb]):
            b = bisect.bisect_right(off_out, q) - 1
            start = off[b] + (q - off_out[b]) * L
            end = min(start + L, off[b + 1])
            most = max(most, end - start)
            acc = Sum(census, "bucket%d" % min(level, 2))
            for e in entries[start:end]:
                acc.add(e)
            out.append(acc.v)
        # the regions are sized by min(in, in / L + NB)
        assert len(out) <= min(len(entries), len(entries) // L + nb)
        if level_outputs is not None:
            level_outputs.append(len(out))
        entries, off = out, off_out
    assert all(off[b + 1] - off[b] <= 1 for b in range(nb))
    # bit partials: segment (j, bit) lists the buckets (j, d) with that bit of d set, entry e <-> d
    # by deleting the bit; chunks of L entries per lane, level after level (kept sparse here: a lane
    # meets its entries in ascending e, which is ascending d, and the absent ones are infinite)
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
                if key not in part:
                    part[key] = Sum(census, "bits0")
                part[key].add(entries[off[bk]])
    most = max(most, min(L, seg_len))
    seg_len, level = -(-seg_len // L), 1
    while seg_len > 1:
        nxt = {}
        for (seg, e), v in part.items():
            if (seg, e // L) not in nxt:
                nxt[seg, e // L] = Sum(census, "bits%d" % min(level, 2))
            nxt[seg, e // L].add(v.v)
        part, seg_len, level = nxt, -(-seg_len // L), level + 1
    assert all(e == 0 for _, e in part)
    tk = [part[k, 0].v if (k, 0) in part else 0 for k in range(nwin * c)]
    if partials is not None:
        partials.extend(tk)
    # final ladder over the W c bit positions
    acc = Sum(census, "final")
    for k in reversed(range(nwin * c)):
        acc.v = 2 * acc.v % R
        if tk[k]:
            acc.add(tk[k])
    return acc.v, most


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


# ------------------------------------------------------------------------------------- the crafted cases
_CENSUS = {}


def case_census(name):
    """[(order, census, T_k)] of one crafted case (tests/msm_cases.py), run once under every order."""
    import msm_cases as M

    if name not in _CENSUS:
        t, runs = M.BY_NAME[name], []
        for order in M.ORDERS:
            census, tk = {}, []
            got, most = msm_model(t.ks, t.scalars, t.c, census=census, partials=tk, order=order)
            assert got == M.dot(t) == expect(t.ks, t.scalars) and most <= L, (name, order)
            # the ladder over the partials is the result, and the arguments change nothing
            assert sum(v << k for k, v in enumerate(tk)) % R == got and len(tk) == -(-256 // t.c) * t.c, (name, order)
            if order is None:
                assert msm_model(t.ks, t.scalars, t.c) == (got, most), name
            runs.append((order, census, tk))
        _CENSUS[name] = runs
    return _CENSUS[name]


def case_names():
    import msm_cases as M
    return [t.name for t in M.CASES]


def test_scatter_orders():
    import msm_cases as M

    assert len(M.ORDERS) >= 8 and len(set(M.ORDERS)) == len(M.ORDERS)
    assert {None, ("index", 0), ("reversed", 0)} < set(M.ORDERS)
    # the orders differ where the device's may: inside a bucket that non-uniform waves fill
    rng = random.Random(1)
    ks = [rng.randrange(1, R) for _ in range(200)]
    seen = set()
    for order in M.ORDERS:
        cnt = [0] * 256
        cnt[9], cnt[10] = 133, 67
        seen.add(tuple(scatter(ks, lambda i, j: 9 if i % 3 else 10, 200, 1, 8, cnt, exscan(cnt), order)))
        assert not any(cnt)
    assert len(seen) == len(M.ORDERS) - 1  # None and "index" agree: both take the points in index order
    # a uniform wave takes its 64 slots with lane l at old - 1 - l: two of them and a tail in one bucket
    cnt = [0] * 256
    cnt[9] = 130
    got = scatter(ks, lambda i, j: 9, 130, 1, 8, cnt, exscan(cnt), ("reversed", 0))
    assert got == ks[:64][::-1] + ks[64:128][::-1] + ks[128:130][::-1]  # the tail wave came first, on top


@pytest.mark.parametrize("name", case_names())
def test_crafted_case_reaches_its_cells(lib, name):
    """Under every scatter order the model computes sum s_i k_i and meets each cell the case is in
    the table for; a c = 8 case is also what the library's own width runs."""
    import msm_cases as M

    t = M.BY_NAME[name]
    if t.c == 8:
        assert lib.kzgpot_msm_window_bits(ctypes.c_uint64(len(t.ks))) == 8
    for order, census, _ in case_census(name):
        for cells in t.must:
            assert all(stage in STAGES and kind in KINDS for stage, kind in cells)
            assert any(census.get(cell) for cell in cells), (name, order, cells, census)
        assert set(census) <= {(s, k) for s in STAGES for k in KINDS}


def test_crafted_cases_cover_every_stage():
    """Every stage x {double, cancel} is some case's required cell, and after_cancel where the order
    of the additions is fixed: the first bit level and the final ladder. (Inside a bucket level it
    depends on the order of the bucket's entries, which the device does not fix.)"""
    import msm_cases as M

    required = {cell for t in M.CASES for cells in t.must if len(cells) == 1 for cell in cells}
    hit = {cell for t in M.CASES for _, census, _ in case_census(t.name) for cell, cnt in census.items() if cnt}
    want = {(s, k) for s in STAGES for k in ("double", "cancel")} | {("bits0", "after_cancel"), ("final", "after_cancel")}
    assert want <= hit
    assert want - {("bucket2", "cancel")} <= required  # that one has an alternative (msm_cases.py)
    # the cancellation at the third bucket level is met by the orders that keep the waves in sequence
    assert all(census.get(("bucket2", "cancel")) for order, census, _ in case_census("bucket2 cancel")
               if order is None or order[0] != "shuffle")
