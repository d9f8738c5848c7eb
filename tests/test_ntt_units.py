"""The Fr NTT's plan (csrc/plans.hpp ntt_plan), its index arithmetic (csrc/ntt_parts.hpp), fr_sub
(csrc/fr.hpp) and the amortized opening's workspace plan (open_domain_plan), driven through a
stand-alone program with its own main (tests/host_units/ntt_units.cpp), built with g++ plain and
under the address + undefined-behaviour sanitizers. No GPU, no HIP header, nothing preloaded: each
binary runs as a child process and must exit 0 without a sanitizer report. The program executes the
plan sequentially through the index functions the kernel uses; every expected value is a Python
integer computed here."""
import os
import random
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host_units", "ntt_units.cpp")
OUT = os.path.join(ROOT, "tests", "host_units", "build")
VARIANTS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined"]}

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TOP = (1 << 256) - 1
EDGES = [0, R - 1, R, R + 1, 2 * R + 1, TOP]
TILES = (8, 9, 10, 11)
MAX_EXP, DOMAIN_MAX_EXP = 26, 24


def omega(exp):
    return pow(7, (R - 1) >> exp, R)


def ntt_ref(x, exp, inverse=False):
    """out[i] = sum_j x[j] w^(ij) (inverse: w^-1 and 1/m): O(m^2) up to exp 6, iterative above."""
    m = 1 << exp
    w = omega(exp)
    if inverse:
        w = pow(w, R - 2, R)
    x = [v % R for v in x]
    if exp <= 6:
        out = [sum(x[j] * pow(w, i * j, R) for j in range(m)) % R for i in range(m)]
    else:
        out = [x[int(f"{i:0{exp}b}"[::-1], 2)] for i in range(m)]
        for q in range(exp):
            h, wq = 1 << q, pow(w, m >> (q + 1), R)
            tw = [1] * h
            for j in range(1, h):
                tw[j] = tw[j - 1] * wq % R
            for base in range(0, m, 2 * h):
                for j in range(h):
                    a, b = out[base + j], out[base + j + h] * tw[j] % R
                    out[base + j], out[base + j + h] = (a + b) % R, (a - b) % R
    if inverse:
        minv = pow(m, R - 2, R)
        out = [v * minv % R for v in out]
    return out


def ntt_inputs(exp, seed):
    """Random 256-bit integers with the edge values at both ends."""
    m = 1 << exp
    rng = random.Random(seed)
    x = [rng.getrandbits(256) for _ in range(m)]
    k = min(len(EDGES), m // 2)
    x[:k] = EDGES[:k]
    if k:
        x[-k:] = EDGES[:k]
    return x


def test_reference_ntt_agrees_with_the_definition():
    x = ntt_inputs(7, 1)
    w = omega(7)
    got = ntt_ref(x, 7)
    for i in (0, 1, 5, 127):
        assert got[i] == sum(v * pow(w, i * j, R) for j, v in enumerate(x)) % R
    assert ntt_ref(got, 7, inverse=True) == [v % R for v in x]


@pytest.fixture(scope="module")
def binaries():
    """The two builds, compiled side by side."""
    os.makedirs(OUT, exist_ok=True)
    procs = {}
    for name, flags in VARIANTS.items():
        exe = os.path.join(OUT, "ntt_units_" + name)
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, SRC, "-o", exe]
        procs[name] = (exe, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    out = {}
    for name, (exe, p) in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, f"{name} build failed:\n{log}"
        out[name] = exe
    return out


def run(exe, lines):
    """The program's answers to `lines`, one per case; fails on a non-zero exit or a sanitizer report."""
    env = dict(os.environ)
    env["UBSAN_OPTIONS"] = "halt_on_error=1 print_stacktrace=1"
    r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=300, env=env)
    report = r.stdout[-2000:] + r.stderr
    assert r.returncode == 0, report[-4000:]
    for mark in ("Sanitizer", "runtime error:"):
        assert mark not in report, report[-4000:]
    got = r.stdout.splitlines()
    assert got[-1] == "ntt_units ok"
    return got[:-1]


def fields(line):
    """key=value tokens -> ({key: int}, {key: [tuple of ints, ...]}) for single and repeated keys."""
    one, many = {}, {}
    for tok in line.split():
        k, v = tok.split("=")
        if "," in v or k in ("pass", "max", "step"):
            many.setdefault(k, []).append(tuple(int(x) for x in v.split(",")))
        else:
            one[k] = int(v)
    return one, many


h = lambda x: f"{x:064x}"  # noqa: E731


# ------------------------------------------------------------------------------------- the transform
def _ntt_cases():
    cases = [(exp, t) for exp in range(14) for t in TILES] + [(14, 8), (16, 8), (17, 8)]
    return [(exp, t, inv) for exp, t in cases for inv in (0, 1)]


@pytest.fixture(scope="module")
def ntt_expected():
    """(inputs, forward, inverse) per exp: the reference is computed once."""
    out = {}
    for exp in sorted({c[0] for c in _ntt_cases()}):
        x = ntt_inputs(exp, 0xA77 + exp)
        out[exp] = (x, ntt_ref(x, exp), ntt_ref(x, exp, inverse=True))
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_plan_executed_on_the_cpu_is_the_ntt(binaries, ntt_expected, variant):
    cases = _ntt_cases()
    lines = []
    for exp, t, inv in cases:
        lines += [f"ntt {exp} {t} {inv}", " ".join(h(v) for v in ntt_expected[exp][0])]
    got = run(binaries[variant], lines)
    assert len(got) == len(cases)
    for (exp, t, inv), line in zip(cases, got):
        assert line.split() == [h(v) for v in ntt_expected[exp][2 if inv else 1]], (exp, t, inv)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fr_sub(binaries, variant):
    rng = random.Random(0x5B)
    special = [0, 1, R - 1, R, R + 1, 2 * R, TOP, (1 << 256) % R]  # test_fr_units.py's special operands
    rand = [rng.getrandbits(256) for _ in range(100)]
    pairs = [(a, b) for a in special for b in special]
    pairs += [(a, rand[(i + 1) % len(rand)]) for i, a in enumerate(rand)]
    pairs += [(a, special[i % len(special)]) for i, a in enumerate(rand)]
    pairs += [(special[i % len(special)], a) for i, a in enumerate(rand)]
    got = run(binaries[variant], [f"sub {h(a)} {h(b)}" for a, b in pairs])
    assert got == [h((a - b) % R) for a, b in pairs]


# ------------------------------------------------------------------------------------- the plans
@pytest.fixture(scope="module")
def plans(binaries):
    keys = [(exp, t) for exp in range(MAX_EXP + 1) for t in TILES]
    got = run(binaries["plain"], [f"plan {exp} {t}" for exp, t in keys])
    return dict(zip(keys, (fields(l) for l in got)))


def test_passes_cover_each_stage_once(plans):
    for (exp, t), (one, many) in plans.items():
        assert one["bytes"] and one["tl"] == min(exp, t)
        stages = []
        for q0, c, lb, stride, blocks in many["pass"]:
            stages += list(range(q0, q0 + c))
            assert c + lb == one["tl"] and stride == 1 << q0 and blocks << one["tl"] == 1 << exp
            assert lb <= q0  # the run's bits lie below the pass's stages
            assert c <= t
        assert stages == list(range(exp)), (exp, t)
        assert len(many["pass"]) == one["npass"] == max(1, -(-exp // t))
    assert [p[1] for p in plans[(17, 8)][1]["pass"]] == [8, 8, 1]
    assert len(plans[(22, 11)][1]["pass"]) == 2 and len(plans[(22, 8)][1]["pass"]) == 3


def test_plan_regions(plans):
    for (exp, t), (one, many) in plans.items():
        assert one["lo_bits"] + one["hi_bits"] == max(0, exp - 1)
        assert one["tw_lo"] == 0 and one["tw_hi"] >= 32 << one["lo_bits"]
        assert one["tw_bytes"] >= one["tw_hi"] + (32 << one["hi_bits"])
        assert one["stage_bytes"] == (32 << exp if one["npass"] > 1 else 0)
        assert one["bytes"] == one["tw_bytes"] + one["stage_bytes"]
        assert one["tw_bytes"] <= 512 << 10  # no table of m / 2 twiddles
        if exp:
            assert one["tw_bytes"] >= plans[(exp - 1, t)][0]["tw_bytes"]


def test_invalid_plans(binaries):
    got = run(binaries["plain"], ["plan 27 11", "plan 10 7", "plan 10 12", "domain 0 25 11", "domain 1 3 12"])
    assert [fields(l)[0]["bytes"] for l in got] == [0] * 5


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_indices_stay_inside_their_regions(binaries, plans, variant):
    keys = list(plans)
    got = run(binaries[variant], [f"bounds {exp} {t}" for exp, t in keys])
    for (exp, t), line in zip(keys, got):
        one, many = plans[(exp, t)]
        maxima = fields(line)[1]["max"]
        assert len(maxima) == one["npass"]
        for load, store, tlo, thi, slot in maxima:
            assert load == store == (1 << exp) - 1  # the largest element is reached and none lies beyond
            assert tlo < 1 << one["lo_bits"] and thi < 1 << one["hi_bits"]
            assert slot < 1 << one["tl"] <= 1 << t
        assert 32 << t <= 65536  # the LDS the kernel declares


def test_open_domain_plan(binaries):
    keys = [(g2, exp, t) for g2 in (0, 1) for exp in range(DOMAIN_MAX_EXP + 1) for t in TILES]
    got = run(binaries["plain"], [f"domain {g2} {exp} {t}" for g2, exp, t in keys])
    prev = {}
    for (g2, exp, t), line in zip(keys, got):
        one, many = fields(line)
        n = 1 << exp
        assert one["ok"] and one["n"] == n and one["rec"] == (192 if g2 else 96)
        assert one["rows"] == (57 if g2 else 29)
        regions = [(one["ntt_in"], 2 * n * 32), (one["scalars"], 2 * n * 32),
                   (one["ntt_tw"], max(one["ntt_tw_bytes"], one["ntt_tw_bytes_out"])),
                   (one["rows_a"], 2 * n * one["rows"] * 4), (one["rows_b"], n * one["rows"] * 4),
                   (one["tw_a"], one["tw_a_bytes"]), (one["tw_b"], one["tw_b_bytes"])]
        assert one["tw_a_bytes"] >= (n + 1) * 32 and one["tw_b_bytes"] >= (n // 2 + 1) * 32
        regions.sort()
        for (o0, s0), (o1, _) in zip(regions, regions[1:]):
            assert o0 + s0 <= o1 and o0 % 256 == 0, (g2, exp, t)
        assert regions[-1][0] + regions[-1][1] <= one["bytes"] == one["ws"]
        # the gather: rows [n - 1, 2n - 1) of the 2n-point buffer -> rows [0, n) of the n-point one
        assert (one["gather_src"], one["gather_dst"], one["gather_cnt"]) == (n - 1, 0, n)
        assert one["gather_src"] + one["gather_cnt"] <= 2 * n and one["gather_dst"] + one["gather_cnt"] <= n
        assert [s[0] for s in many["step"]] == list(range(8))
        assert one["bytes"] > prev.get((g2, t), 0) and one["table_ws"] > prev.get((g2, t, "table"), 0)
        prev[(g2, t)], prev[(g2, t, "table")] = one["bytes"], one["table_ws"]
