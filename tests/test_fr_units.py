"""The scalar field module (csrc/fr.hpp: load / store, mul, add, pow, inverse, the exponents, the
domain roots, the x^(2^k) table, both byte orders) driven through a stand-alone program with its own
main (tests/host_units/fr_units.cpp), built with g++ plain and under the address +
undefined-behaviour sanitizers. No GPU, no HIP header, nothing preloaded: each binary runs as a
child process, reads the cases from stdin, and must exit 0 without a sanitizer report; every
expected value is a Python integer computed here."""
import os
import random
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host_units", "fr_units.cpp")
OUT = os.path.join(ROOT, "tests", "host_units", "build")
VARIANTS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined"]}

R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
TOP = (1 << 256) - 1


def _cases():
    """(input line, expected output line) pairs."""
    r = R_MOD
    rng = random.Random(0xF12)
    special = [0, 1, r - 1, r, r + 1, 2 * r, TOP, (1 << 256) % r]
    rand = [rng.getrandbits(256) for _ in range(200)]
    ops = special + rand
    h = lambda x: f"{x:064x}"
    cases = [("one", h((1 << 256) % r)), ("rm2", h(r - 2))]
    for a in ops:
        cases.append((f"load {h(a)}", h(a % r)))
        cases.append((f"inv {h(a)}", h(pow(a, r - 2, r))))
        v = a % r
        cases.append((f"bytes {h(a)}", v.to_bytes(32, "little").hex() + " " + v.to_bytes(32, "big").hex()))
    # every pair of the special operands, every random one with another and with a special one
    pairs = [(a, b) for a in special for b in special]
    pairs += [(a, rand[(i + 1) % len(rand)]) for i, a in enumerate(rand)]
    pairs += [(a, special[i % len(special)]) for i, a in enumerate(rand)]
    for a, b in pairs:
        cases.append((f"mul {h(a)} {h(b)}", h(a * b % r)))
        cases.append((f"add {h(a)} {h(b)}", h((a + b) % r)))
    shifted = [(r - 1) >> k for k in range(33)]
    for a in special + rand[:8]:
        for e in [0, 1, r - 2, TOP] + shifted:
            cases.append((f"pow {h(a)} {h(e)}", h(pow(a, e, r))))
    for k in range(33):
        cases.append((f"rm1shr {k}", h(shifted[k])))
        cases.append((f"root {k}", h(pow(7, shifted[k], r))))
    for x in (rand[0], TOP):
        row, p = [], x % r
        for _ in range(64):
            row.append(h(p))
            p = p * p % r
        cases.append((f"table {h(x)}", " ".join(row)))
    return cases


@pytest.fixture(scope="module")
def binaries():
    """The two builds, compiled side by side."""
    os.makedirs(OUT, exist_ok=True)
    procs = {}
    for name, flags in VARIANTS.items():
        exe = os.path.join(OUT, "fr_units_" + name)
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, SRC, "-o", exe]
        procs[name] = (exe, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    out = {}
    for name, (exe, p) in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, f"{name} build failed:\n{log}"
        out[name] = exe
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fr_units(binaries, cases, variant):
    env = dict(os.environ)
    # a sanitizer finding ends the run with a non-zero exit code instead of only a report
    env["UBSAN_OPTIONS"] = "halt_on_error=1 print_stacktrace=1"
    stdin = "".join(line + "\n" for line, _ in cases)
    r = subprocess.run([binaries[variant]], input=stdin, capture_output=True, text=True, timeout=60, env=env)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-4000:]
    for mark in ("Sanitizer", "runtime error:"):
        assert mark not in report, report[-4000:]
    got = r.stdout.splitlines()
    assert got[-1] == "fr_units ok" and len(got) == len(cases) + 1
    for (line, want), have in zip(cases, got):
        assert have == want, line
