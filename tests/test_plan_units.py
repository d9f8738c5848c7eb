"""The launch plans (csrc/plans.hpp: the workspace layouts and launch schedules of the group FFT, the
multi-scalar multiplication, the polynomial division and KZG10 open) driven through a stand-alone
program with its own main (tests/host_units/plan_units.cpp), built with g++ plain and under the
address + undefined-behaviour sanitizers. No GPU, no HIP header, nothing preloaded: each binary runs
as a child process, reads the cases from stdin, prints every plan with its schedule, and must exit 0
without a sanitizer report. Everything a launch reads and writes is then checked here against the
regions the plan gives it, with the expected geometry computed in Python."""
import ctypes
import os
import random
import subprocess
from collections import Counter

import pytest

from conftest import ROOT
from test_msm_model import R, msm_model, scalar_sets
from test_poly_open_host import boundary_sizes

SRC = os.path.join(ROOT, "tests", "host_units", "plan_units.cpp")
OUT = os.path.join(ROOT, "tests", "host_units", "build")
VARIANTS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined"]}

L = 64
NONE = (1 << 64) - 1
MSM_MAX_N = 1 << 26
POLY_MAX_N = (1 << 26) + 1

MSM_NS = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, (1 << 18) + 1, 1 << 20, (1 << 24) + 1, 1 << 26]
MSM_REJECTED = [(MSM_MAX_N + 1, 8), (1000, 17), (1 << 26, 1)]
# the (n, c) tests/test_msm_model.py runs its model at (the library's width is 8 up to n = 28415)
MODEL_CASES = [(70, c) for c in range(1, 17)] + [(n, 8) for n in (1, 2, 63, 64, 65, 1000)]
# test_poly_open_host.py test_workspaces_are_monotone_in_n
OPEN_NS = [0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 65536, 65537, 1 << 20, (1 << 20) + 1, 1 << 22,
           (1 << 24) + 1, 1 << 26, POLY_MAX_N]
OPEN_CASES = ([(n, nb, 0) for nb in (0, 3, 1024) for n in OPEN_NS if n - 1 + nb - 1 <= 1 << 26]
              + [(1 << 16, nb, 0) for nb in OPEN_NS[:14]] + [(1 << 16, 0, 0), (1 << 16, 0, 1)])
# tests/test_msm_model.py test_window_bits_and_workspace
WS_NS = [0, 1, 2, 63, 64, 65, 1000, 4097, 1 << 16, (1 << 20) + 1, 1 << 22, 1 << 26]


def msm_line(g2, n, c):
    return f"msm {g2} {n} {c}"


def all_lines():
    lines = [msm_line(g2, n, c) for g2 in (0, 1) for n in MSM_NS for c in range(1, 17)]
    lines += [msm_line(g2, n, c) for g2 in (0, 1) for n, c in MSM_REJECTED]
    lines += [msm_line(0, n, c) for n, c in MODEL_CASES]
    lines += [f"msmws {g2} {n} {flags}" for g2 in (0, 1) for n in WS_NS + [MSM_MAX_N + 1]
              for flags in (0, 1, 12 << 8, 17 << 8, 2)]
    lines += [f"poly {n} {t}" for t in range(8, 13) for n in boundary_sizes(t) + [POLY_MAX_N]]
    lines += [f"poly {POLY_MAX_N + 1} 11", "poly 1000 7", "poly 1000 13"]
    lines += [f"fft {g2} {exp} {inv}" for g2 in (0, 1) for exp in range(34) for inv in (0, 1)]
    for n, nb, flags in OPEN_CASES:  # the plan, and the sizes of what it stacks
        lines += [f"open {n} {nb} {flags}", f"poly {max(n, nb)} 11", f"msmws 0 {max(n - 1, 0) + max(nb - 1, 0)} {flags}"]
    lines += [f"grid {n} {b}" for n in (0, 1, 255, 256, 257, (1 << 32) - 1) for b in (128, 256)]
    return list(dict.fromkeys(lines))


def parse(line):
    """key=value tokens -> {key: int}; the repeated keys (step, level, stage) -> lists of int tuples"""
    out = {}
    for tok in line.split():
        k, v = tok.split("=")
        if k in ("step", "level", "stage"):
            out.setdefault(k + "s", []).append(tuple(int(x) for x in v.split(",")))
        else:
            out[k] = int(v)
    return out


@pytest.fixture(scope="module")
def binaries():
    """The two builds, compiled side by side."""
    os.makedirs(OUT, exist_ok=True)
    procs = {}
    for name, flags in VARIANTS.items():
        exe = os.path.join(OUT, "plan_units_" + name)
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, SRC, "-o", exe]
        procs[name] = (exe, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    out = {}
    for name, (exe, p) in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, f"{name} build failed:\n{log}"
        assert "warning" not in log, log
        out[name] = exe
    return out


@pytest.fixture(scope="module")
def plans(binaries):
    """{variant: {case line: parsed answer}}: each binary run once over every case"""
    lines = all_lines()
    env = dict(os.environ)
    # a sanitizer finding ends the run with a non-zero exit code instead of only a report
    env["UBSAN_OPTIONS"] = "halt_on_error=1 print_stacktrace=1"
    out = {}
    for variant, exe in binaries.items():
        r = subprocess.run([exe], input="".join(x + "\n" for x in lines), capture_output=True, text=True, timeout=60,
                           env=env)
        report = r.stdout + r.stderr
        assert r.returncode == 0, report[-4000:]
        for mark in ("Sanitizer", "runtime error:"):
            assert mark not in report, report[-4000:]
        got = r.stdout.splitlines()
        assert got[-1] == "plan_units ok" and len(got) == len(lines) + 1
        out[variant] = {line: parse(have) for line, have in zip(lines, got)}
    return out


def align256(x):
    return (x + 255) & ~255


def assert_regions(regions, total, where):
    """(name, start, bytes used) triples: 256-aligned, disjoint, inside [0, total)"""
    regions = sorted(regions, key=lambda r: r[1])
    for name, start, used in regions:
        assert start % 256 == 0, (where, name)
    for (name, start, used), (_, nxt, _) in zip(regions, regions[1:] + [("end", total, 0)]):
        assert start + used <= nxt, (where, name)


# ------------------------------------------------------------------------------------- MSM
def bucket_distributions(n, c):
    """Bucket counts {entries: buckets} of one window that holds all n points."""
    nbk = (1 << c) - 1
    q, r = divmod(n, nbk)
    even = Counter({q + 1: r, q: nbk - r})
    k = min(nbk, n // (L + 1))
    rest = n - k * (L + 1)
    if k < nbk:
        full = Counter({L + 1: k}) + Counter({rest: 1})
    else:  # every bucket has L + 1; the remainder joins one of them
        full = Counter({L + 1: k - 1}) + Counter({L + 1 + rest: 1})
    dists = {"one bucket": Counter({n: 1}), "even": even, "L + 1 each": full}
    for name, d in dists.items():
        d = dists[name] = Counter({cnt: mult for cnt, mult in d.items() if cnt and mult})
        assert sum(cnt * mult for cnt, mult in d.items()) == n and sum(d.values()) <= nbk
    return dists


def check_msm(p, g2, n, c, where):
    nwin = -(-256 // c)
    assert p["ok"] == (1 if n * nwin < 1 << 32 else 0), where
    if not p["ok"]:
        assert p["bytes"] == 0, where
        return
    nb, nseg, entries = nwin << c, nwin * c, n * nwin
    assert (p["c"], p["nwin"], p["nb"], p["nseg"], p["entries"]) == (c, nwin, nb, nseg, entries), where
    assert p["chunk"] == L and p["rows"] == (57 if g2 else 29), where
    # the scan: ntiles tiles cover the buckets, and one tile covers the tile sums
    assert p["ntiles"] * p["scan_tile"] >= nb and p["ntiles"] <= p["scan_tile"], where
    assert_regions([("cnt", p["cnt"], nb * 4), ("off_a", p["off_a"], (nb + 1) * 4), ("off_b", p["off_b"], (nb + 1) * 4),
                    ("sums", p["sums"], (p["ntiles"] + 1) * 4), ("idx", p["idx"], entries * 4),
                    ("pool", p["pool"], p["cap"] * p["rows"] * 4)], p["bytes"], where)
    # the pool: n bases, then A, then B
    assert n <= p["base_a"] <= p["base_b"] <= p["cap"], where
    region = {"A": (p["base_a"], p["base_b"]), "B": (p["base_b"], p["cap"])}

    def region_of(lo, hi):
        inside = [name for name, (a, b) in region.items() if a <= lo and hi <= b]
        assert len(inside) >= 1, (where, lo, hi)
        return inside[0] if lo < hi else None  # an empty range lies nowhere

    steps = p["steps"]
    levels = p["levels"]
    assert len(steps) == p["nsteps"] and 1 <= levels <= 6 and 1 <= len(steps) - levels <= 3, where
    assert [s[0] for s in steps] == [0] + [1] * (levels - 1) + [2] + [3] * (len(steps) - levels - 1), where
    assert L ** levels >= n and (levels == 1 or L ** (levels - 1) < n), where
    prev = None
    for k, (mode, in_base, out_base, lanes, s_nseg, seg_len, seg_chunks, off_in, off_out) in enumerate(steps):
        wrote = region_of(out_base, out_base + lanes)
        if mode == 0:
            assert in_base == 0, where  # reads the bases [0, n) through idx, below both regions
        else:
            p_out, p_lanes = prev[2], prev[3]
            assert in_base == p_out, where
            read = region_of(in_base, in_base + p_lanes)
            assert read is None or wrote is None or read != wrote, (where, k)
        if mode < 2:
            assert {off_in, off_out} == {p["off_a"], p["off_b"]} and off_in != off_out, (where, k)
            assert off_in == (prev[8] if prev else p["off_a"]), (where, k)  # the prologue scans into off_a
        else:
            assert off_in == steps[levels - 1][8] and off_out == NONE, (where, k)
            assert s_nseg == nseg and seg_chunks == -(-seg_len // L) and lanes == nseg * seg_chunks, (where, k)
            if mode == 2:
                assert seg_len == 1 << (c - 1), where
            else:  # reads exactly what the step before wrote
                assert seg_len == prev[6] and nseg * seg_len == prev[3], (where, k)
        prev = steps[k]
    assert steps[-1][6] == 1 and steps[-1][3] == nseg, where  # one entry per segment is left
    assert p["final_base"] == steps[-1][2], where
    assert region_of(p["final_base"], p["final_base"] + nseg) is not None, where
    # the lane counts hold whatever the scalars are
    for name, dist in bucket_distributions(n, c).items():
        for k in range(levels):
            nxt = Counter()
            for cnt, mult in dist.items():
                nxt[-(-cnt // L)] += mult
            dist = nxt
            assert nwin * sum(cnt * mult for cnt, mult in dist.items()) <= steps[k][3], (where, name, k)
        assert all(cnt <= 1 for cnt in dist), (where, name)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_msm_plans(plans, variant):
    for g2 in (0, 1):
        for n in MSM_NS:
            for c in range(1, 17):
                check_msm(plans[variant][msm_line(g2, n, c)], g2, n, c, (g2, n, c))
        for n, c in MSM_REJECTED:
            p = plans[variant][msm_line(g2, n, c)]
            assert p["ok"] == 0 and p["bytes"] == 0, (g2, n, c)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_msm_workspace_sizes(plans, variant, kzgpot_mod):
    """msm_workspace_bytes: the explicit width's plan, the maximum over 8 .. the library's width for
    c = 0, nothing for invalid flags — and what the library itself reports."""
    from kzgpot import _lib

    lib = _lib.load()
    for g2 in (0, 1):
        for n in WS_NS + [MSM_MAX_N + 1]:
            for flags in (0, 1, 12 << 8, 17 << 8, 2):
                got = plans[variant][f"msmws {g2} {n} {flags}"]
                assert got["bytes"] == lib.kzgpot_msm_workspace(g2, ctypes.c_uint64(n), flags), (g2, n, flags)
                assert got["width"] == lib.kzgpot_msm_window_bits(ctypes.c_uint64(n))
                if n in MSM_NS and flags == 12 << 8:
                    assert got["bytes"] == plans[variant][msm_line(g2, n, 12)]["bytes"]
                if n in MSM_NS and flags == 0:
                    want = max(plans[variant][msm_line(g2, n, w)]["bytes"] for w in range(8, got["width"] + 1))
                    assert got["bytes"] == want, (g2, n)
                if flags in (17 << 8, 2) or n > MSM_MAX_N:
                    assert got["bytes"] == 0


def test_msm_model_stays_within_the_plan(plans):
    """The schedule's model (test_msm_model.py) writes no more partial sums per level, in no more
    levels, than the C++ plan launches lanes for."""
    for n, c in MODEL_CASES:
        p = plans["plain"][msm_line(0, n, c)]
        rng = random.Random(n * 17 + c)
        ks = [rng.randrange(1, R) for _ in range(n)]
        for name, s in scalar_sets(rng, n).items():
            outputs = []
            msm_model(ks, s, c, outputs)
            assert len(outputs) == p["levels"], (n, c, name)
            for k, wrote in enumerate(outputs):
                assert wrote <= p["steps"][k][3], (n, c, name, k)


# ------------------------------------------------------------------------------------- division
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_poly_plans(plans, variant):
    for t in range(8, 13):
        S = 1 << t
        for n in boundary_sizes(t) + [POLY_MAX_N]:
            p = plans[variant][f"poly {n} {t}"]
            levels = p["levels"]
            assert p["top"] + 1 == len(levels) == 1 + (n > S) + (n > S * S) + (n > S * S * S), (t, n)
            assert levels[0][0] == n, (t, n)
            assert_regions([(k, off, cnt * 32) for k, (cnt, off, _, _) in enumerate(levels) if k], p["bytes"], (t, n))
            for k, (cnt, off, tiles, pow0) in enumerate(levels):
                assert tiles == -(-cnt // S), (t, n, k)
                if k + 1 < len(levels):
                    assert levels[k + 1][0] == tiles, (t, n, k)
                else:
                    assert tiles == 1, (t, n)  # the top level fits one tile
                assert pow0 == k * t and pow0 + p["reads"] <= p["powers"], (t, n, k)
    for line in (f"poly {POLY_MAX_N + 1} 11", "poly 1000 7", "poly 1000 13"):
        assert plans[variant][line]["bytes"] == 0, line


# ------------------------------------------------------------------------------------- group FFT
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fft_plans(plans, variant):
    for g2 in (0, 1):
        for inv in (0, 1):
            for exp in range(33):
                p = plans[variant][f"fft {g2} {exp} {inv}"]
                m, half = 1 << exp, (1 << exp) >> 1
                assert p["ok"] and (p["m"], p["half"]) == (m, half), (g2, exp)
                # m/2 + 1 twiddles of 32 B, then 2 NW + 1 rows of m words
                assert p["work"] == p["twiddle_bytes"] == align256((half + 1) * 32), (g2, exp)
                assert p["rows"] == (57 if g2 else 29), (g2, exp)
                assert p["bytes"] == p["workspace_bytes"] == p["work"] + m * p["rows"] * 4, (g2, exp)
                stages = p.get("stages", [])
                assert len(stages) == p["nstages"] == exp, (g2, exp)
                assert [logh for _, logh, _ in stages] == list(range(exp)), (g2, exp)
                for lognb, logh, uniform in stages:
                    assert lognb + logh + 1 == exp and uniform == (1 if lognb >= 6 else 0), (g2, exp, logh)
                    # butterfly t < m/2: j = t >> lognb, k = t & (nb - 1) (k_fft_stage); the largest of each
                    j, k = (half - 1) >> lognb, min(half - 1, (1 << lognb) - 1)
                    i1 = (k << (logh + 1)) + j + (1 << logh)
                    assert i1 < m and (j << lognb) < half, (g2, exp, logh)
                assert p["scale"] == (1 if inv and exp else 0), (g2, exp)
            assert plans[variant][f"fft {g2} 33 {inv}"] == {"ok": 0, "bytes": 0}


# ------------------------------------------------------------------------------------- open
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_open_plans(plans, variant):
    for n, nb_in, flags in OPEN_CASES:
        p = plans[variant][f"open {n} {nb_in} {flags}"]
        where = (n, nb_in, flags)
        assert p["ok"], where
        nq, nb = max(n - 1, 0), max(nb_in - 1, 0)
        assert (p["nq"], p["nb"], p["rec"], p["t"], p["c"]) == (nq, nb, 104 if flags & 1 else 96, 11, 0), where
        assert p["poly_ws"] == plans[variant][f"poly {max(n, nb_in)} 11"]["bytes"] >= 256, where
        assert p["msm_ws"] == plans[variant][f"msmws 0 {nq + nb} {flags}"]["bytes"] > 0, where
        assert_regions([("bases", p["bases"], (nq + nb) * p["rec"]), ("scalars", p["scalars"], (nq + nb) * 32),
                        ("values", p["values"], 64), ("poly", p["poly"], p["poly_ws"]),
                        ("msm", p["msm"], p["msm_ws"])], p["bytes"], where)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_grid_for(plans, variant):
    for n in (0, 1, 255, 256, 257, (1 << 32) - 1):
        for b in (128, 256):
            assert plans[variant][f"grid {n} {b}"]["blocks"] == max(1, -(-n // b)), (n, b)
