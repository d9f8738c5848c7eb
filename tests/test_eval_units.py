"""The evaluation-form plans (csrc/plans.hpp eval_plan, open_evals_plan) and the host side of the
division in evaluation form (csrc/fr.hpp: z^n, 1/n, the table of w^(2^k)), driven through a
stand-alone program with its own main (tests/host_units/eval_units.cpp), built with g++ plain and
under the address + undefined-behaviour sanitizers. No GPU, no HIP header, nothing preloaded: each
binary runs as a child process and must exit 0 without a sanitizer report. Every expected value is a
Python integer computed here. The library's workspace functions and argument checks are host-only,
so they are checked against the same plans without a GPU."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host_units", "eval_units.cpp")
OUT = os.path.join(ROOT, "tests", "host_units", "build")
VARIANTS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined"]}

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TOP = (1 << 256) - 1
TILES = (8, 9, 10, 11, 12)
MAX_EXP = 26
E_INVALID_ARG = -100


def omega(exp):
    return pow(7, (R - 1) >> exp, R)


@pytest.fixture(scope="module")
def binaries():
    """The two builds, compiled side by side."""
    os.makedirs(OUT, exist_ok=True)
    procs = {}
    for name, flags in VARIANTS.items():
        exe = os.path.join(OUT, "eval_units_" + name)
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
    assert got[-1] == "eval_units ok"
    return got[:-1]


def fields(line):
    return {k: int(v) for k, v in (tok.split("=") for tok in line.split())}


h = lambda x: f"{x:064x}"  # noqa: E731


# ------------------------------------------------------------------------------------- the plans
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_eval_plan(binaries, kzgpot_mod, variant):
    keys = [(exp, t) for exp in range(MAX_EXP + 1) for t in TILES]
    got = run(binaries[variant], [f"plan {exp} {t}" for exp, t in keys])
    prev = {}
    for (exp, t), line in zip(keys, got):
        p = fields(line)
        n = 1 << exp
        assert (p["exp"], p["t"], p["n"]) == (exp, t, n)
        assert p["tiles"] == -(-n // (1 << t)) >= 1
        regions = sorted([(p["inv"], 32 * n), (p["sums"], 32 * p["tiles"]), (p["qsums"], 32 * p["tiles"]),
                          (p["words"], 256)])
        for (o0, s0), (o1, _) in zip(regions, regions[1:]):
            assert o0 % 256 == 0 and o0 + s0 <= o1, (exp, t)
        assert regions[-1][0] % 256 == 0 and regions[-1][0] + regions[-1][1] <= p["bytes"] == p["ws"]
        assert p["value_at"] >= 4 and p["value_at"] + 32 <= 256 and p["value_at"] % 16 == 0  # beside the index word
        # the loaded library reports the plan's size; tile 0 is the library's (2^11)
        assert kzgpot_mod.fr_evals_workspace(exp, t << 16) == p["bytes"]
        if t == 11:
            assert kzgpot_mod.fr_evals_workspace(exp, 0) == p["bytes"]
        assert p["bytes"] >= prev.get(t, 0)  # monotone in exp
        prev[t] = p["bytes"]


def test_rejected_plans(binaries, kzgpot_mod):
    got = run(binaries["plain"], ["plan 27 11", "plan 10 7", "plan 10 13", "open 27 0", "open 10 458752", "open 10 2",
                                  f"open 10 {17 << 8}", f"tiles {(1 << 26) + 1} 11", "tiles 100 7", "tiles 100 13"])
    assert [fields(l)["bytes"] for l in got[:6 + 1]] == [0] * 7
    assert [fields(l)["tiles"] for l in got[7:]] == [0] * 3
    k = kzgpot_mod
    for tile in (1, 7, 13, 15):
        assert k.fr_evals_workspace(10, tile << 16) == 0 and k.kzg_open_evals_workspace(10, tile << 16) == 0
    for flags in (1, 1 << 8, 1 << 15, 1 << 20, 1 << 31):  # the MSM's flags are not the division's
        assert k.fr_evals_workspace(10, flags) == 0
    for flags in (2, 1 << 13, 1 << 20, 1 << 31, 17 << 8):  # unknown bits; a window width above 16
        assert k.kzg_open_evals_workspace(10, flags) == 0
    assert k.fr_evals_workspace(27) == 0 and k.kzg_open_evals_workspace(27) == 0
    assert k.fr_evals_workspace(26) > 0 and k.kzg_open_evals_workspace(26) > 0
    assert k.kzg_open_evals_workspace(26, 3 << 8) == 0  # 2^26 bases at width 3: above the MSM's limit


def test_batch_inverse_tiles(binaries):
    cases = [(n, t) for t in TILES for n in (0, 1, (1 << t) - 1, 1 << t, (1 << t) + 1, 65537, 1 << 26)]
    got = run(binaries["asan_ubsan"], [f"tiles {n} {t}" for n, t in cases])
    assert [fields(l)["tiles"] for l in got] == [-(-n // (1 << t)) for n, t in cases]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_open_evals_plan(binaries, kzgpot_mod, variant):
    keys = [(exp, t, c, mont) for exp in (0, 1, 5, 10, 16, 20, 26) for t in (0, 8, 12) for c in (0, 5, 16)
            for mont in (0, 1)]
    keys = [k for k in keys if kzgpot_mod.msm_workspace(False, 1 << k[0], k[2] << 8)]
    assert len(keys) > 100
    flags = lambda t, c, mont: mont | c << 8 | t << 16  # noqa: E731
    got = run(binaries[variant], [f"open {exp} {flags(t, c, mont)}" for exp, t, c, mont in keys])
    plans = dict(zip(keys, got))
    for (exp, t, c, mont), line in plans.items():
        p = fields(line)
        n = 1 << exp
        assert p["ok"] and (p["n"], p["t"], p["c"], p["rec"]) == (n, t or 11, c, 104 if mont else 96)
        assert p["ev_bytes"] == kzgpot_mod.fr_evals_workspace(exp, t << 16)
        assert p["msm_bytes"] == kzgpot_mod.msm_workspace(False, n, mont | c << 8)
        # the division's workspace, the quotient, the MSM's workspace: in that order, none overlapping
        assert p["ev_bytes"] <= p["quot"] and p["quot"] + 32 * n <= p["msm"] and p["msm"] + p["msm_bytes"] <= p["bytes"]
        assert p["quot"] % 256 == 0 and p["msm"] % 256 == 0
        assert kzgpot_mod.kzg_open_evals_workspace(exp, flags(t, c, mont)) == p["bytes"]


# ------------------------------------------------------------------------------------- the host's Fr helpers
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_host_scalars(binaries, variant):
    rng = random.Random(0xE7A1)
    cases = []
    for exp in (0, 1, 8, 26):
        n, w = 1 << exp, omega(exp)
        cases += [(exp, z) for z in (0, 1, w, pow(w, n - 1, R), R - 1, R, TOP, rng.getrandbits(256))]
    got = run(binaries[variant], [f"host {exp} {h(z)}" for exp, z in cases])
    for (exp, z), line in zip(cases, got):
        n, w, zr = 1 << exp, omega(exp), z % R
        zn = pow(zr, n, R)
        ninv = pow(n, R - 2, R)
        want = [zr, zn, ninv, (zn - 1) * ninv % R] + [pow(w, 1 << k, R) for k in range(26)]
        assert line.split() == [h(v) for v in want], (exp, hex(z))
        assert ninv * n % R == 1 and pow(w, n, R) == 1 and (exp == 0 or pow(w, n // 2, R) == R - 1)
        # the barycentric factor vanishes exactly on the domain
        assert (want[3] == 0) == (zn == 1)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_binary_inversion(binaries, variant):
    """fr_inv_binary (what a tile's one inversion runs) against pow(a, r - 2, r) and against fr_inv."""
    rng = random.Random(0xB1)
    vals = [0, 1, 2, 3, R - 1, R - 2, R, R + 1, 2 * R + 1, TOP, (R + 1) // 2, 1 << 254, (1 << 254) + 1, (1 << 256) % R,
            pow((1 << 256) % R, R - 2, R)]
    vals += [1 << k for k in range(0, 256, 17)] + [(1 << k) - 1 for k in range(2, 256, 19)]
    vals += [rng.getrandbits(256) for _ in range(300 if variant == "plain" else 60)] + [rng.getrandbits(64) for _ in range(20)]
    got = run(binaries[variant], [f"inv {h(a)}" for a in vals])
    for a, line in zip(vals, got):
        want = h(pow(a % R, R - 2, R))
        assert line.split() == [want, want], hex(a)


# ------------------------------------------------------------------------------------- the formulas
def horner(coeffs, z):
    """(quotient, value) of the division by (x - z)."""
    hs, acc = [0] * len(coeffs), 0
    for j in range(len(coeffs) - 1, -1, -1):
        acc = (acc * z + coeffs[j]) % R
        hs[j] = acc
    return hs[1:], hs[0]


def evaluate(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


@pytest.mark.parametrize("exp", [0, 1, 2, 3, 4, 5])
def test_formulas_in_python(exp):
    """The two formulas of include/kzgpot.h (z off the domain, z = w^m) against Horner and
    re-evaluation, in Python integers alone; n = 1 included, where z = 1 is on the domain and the
    quotient is [0]."""
    n, w = 1 << exp, omega(exp)
    rng = random.Random(exp)
    c = [rng.randrange(R) for _ in range(n)]
    ws = [pow(w, i, R) for i in range(n)]
    e = [evaluate(c, x) for x in ws]
    inv = lambda a: pow(a % R, R - 2, R)  # noqa: E731
    for z in [12345, 0, R - 1] + ws:
        q, v = horner(c, z)
        want = [evaluate(q, x) for x in ws]
        if pow(z, n, R) != 1:
            value = (pow(z, n, R) - 1) * inv(n) * sum(e[i] * ws[i] * inv(z - ws[i]) for i in range(n)) % R
            got = [(value - e[i]) * inv(z - ws[i]) % R for i in range(n)]
        else:
            m = ws.index(z)
            value = e[m]
            got = [(value - e[i]) * inv(z - ws[i]) % R if i != m else 0 for i in range(n)]
            got[m] = -sum(got[i] * pow(w, (i - m) % n, R) for i in range(n) if i != m) % R
        assert (value, got) == (v, want), (exp, z)
    if exp == 0:
        assert ws == [1] and horner(c, 1) == ([], c[0])  # the quotient polynomial is 0: its one evaluation is 0


# ------------------------------------------------------------------------------------- argument errors
def test_invalid_arguments_return_before_any_device_use(kzgpot_mod):
    """Every case is decided on the host: -100 with or without a GPU, and the outputs stay as they were."""
    from kzgpot import _lib

    lib = _lib.load()
    z = (5).to_bytes(32, "little")
    buf = b"\x01" * (32 * 16)
    pts = b"\x00" * (96 * 16)
    out = ctypes.create_string_buffer(b"\xab" * 512, 512)
    val = ctypes.create_string_buffer(b"\xab" * 32, 32)
    fb = ctypes.c_int64(-1)
    untouched = lambda: out.raw == b"\xab" * 512 and val.raw == b"\xab" * 32  # noqa: E731

    inv = lib.kzgpot_fr_batch_inverse
    assert inv(None, 16, out, 0) == E_INVALID_ARG
    assert inv(buf, 16, None, 0) == E_INVALID_ARG
    assert inv(buf, (1 << 26) + 1, out, 0) == E_INVALID_ARG
    for flags in (1, 1 << 8, 7 << 16, 13 << 16, 1 << 20):
        assert inv(buf, 16, out, flags) == E_INVALID_ARG
    assert inv(None, 0, None, 0) == 0  # nothing to do, no pointer needed
    assert lib.kzgpot_fr_batch_inverse_dev(None, 16, out, 0, None) == E_INVALID_ARG
    assert lib.kzgpot_fr_batch_inverse_dev(buf, 16, out, 13 << 16, None) == E_INVALID_ARG

    div = lib.kzgpot_fr_evals_divide
    assert div(None, 4, z, out, val, 0) == E_INVALID_ARG
    assert div(buf, 4, None, out, val, 0) == E_INVALID_ARG
    assert div(buf, 4, z, out, None, 0) == E_INVALID_ARG
    assert div(buf, 27, z, out, val, 0) == E_INVALID_ARG
    for flags in (1, 1 << 8, 7 << 16, 13 << 16, 1 << 20):
        assert div(buf, 4, z, out, val, flags) == E_INVALID_ARG
    ddiv = lib.kzgpot_fr_evals_divide_dev
    assert ddiv(buf, 4, z, out, val, 0, None, None) == E_INVALID_ARG  # no workspace
    assert ddiv(None, 4, z, out, val, 0, out, None) == E_INVALID_ARG
    assert ddiv(buf, 27, z, out, val, 0, out, None) == E_INVALID_ARG
    assert ddiv(buf, 4, z, out, val, 1, out, None) == E_INVALID_ARG

    opn = lib.kzgpot_g1_kzg_open_evals
    assert opn(None, buf, 4, z, out, 0, ctypes.byref(fb)) == E_INVALID_ARG
    assert opn(pts, None, 4, z, out, 0, ctypes.byref(fb)) == E_INVALID_ARG
    assert opn(pts, buf, 4, None, out, 0, ctypes.byref(fb)) == E_INVALID_ARG
    assert opn(pts, buf, 4, z, None, 0, ctypes.byref(fb)) == E_INVALID_ARG
    assert opn(pts, buf, 27, z, out, 0, ctypes.byref(fb)) == E_INVALID_ARG
    for flags in (2, 1 << 13, 17 << 8, 7 << 16, 13 << 16, 1 << 20):
        assert opn(pts, buf, 4, z, out, flags, ctypes.byref(fb)) == E_INVALID_ARG
    dopn = lib.kzgpot_g1_kzg_open_evals_dev
    assert dopn(pts, buf, 4, z, out, 0, None, val, None) == E_INVALID_ARG  # no workspace
    assert dopn(pts, buf, 4, z, out, 0, out, None, None) == E_INVALID_ARG  # no key
    assert dopn(pts, buf, 27, z, out, 0, out, val, None) == E_INVALID_ARG
    assert dopn(pts, buf, 4, z, out, 2, out, val, None) == E_INVALID_ARG
    assert untouched() and fb.value == -1

    k = kzgpot_mod
    with pytest.raises(ValueError):
        k.fr_evals_divide([1, 2, 3], 2, 5)  # not 2^exp values
    with pytest.raises(ValueError):
        k.fr_evals_divide([1], 27, 5)
    with pytest.raises(ValueError):
        k.kzg_open_evals(pts, [1] * 8, 4, 5)
    with pytest.raises(ValueError):
        k.fr_batch_inverse(b"\x00" * 33)
    with pytest.raises(ValueError):
        k.fr_batch_inverse([1], tile=16)
