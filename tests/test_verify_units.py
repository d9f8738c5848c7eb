"""The launch plans of the pairing product and of KZG10 check / batch_check (csrc/plans.hpp
pairing_plan, check_plan), driven through a stand-alone program with its own main
(tests/host_units/verify_units.cpp), built with g++ plain and under the address + undefined-behaviour
sanitizers. No GPU, no HIP header, nothing preloaded: each binary runs as a child process and must exit
0 without a sanitizer report. The library's workspace functions and argument checks are host-only, so
they are checked against the same plans without a GPU."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host_units", "verify_units.cpp")
OUT = os.path.join(ROOT, "tests", "host_units", "build")
VARIANTS = {"plain": [], "asan_ubsan": ["-fsanitize=address,undefined"]}

E_INVALID_ARG = -100
MAX_PAIRS = 1 << 16
MAX_N = (1 << 25) - 1
CHECK_NS = (0, 1, 255, 256, 257, MAX_N)  # around the Fr kernel's block of 256, and both ends


@pytest.fixture(scope="module")
def binaries():
    os.makedirs(OUT, exist_ok=True)
    procs = {}
    for name, flags in VARIANTS.items():
        exe = os.path.join(OUT, "verify_units_" + name)
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, SRC, "-o", exe]
        procs[name] = (exe, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    out = {}
    for name, (exe, p) in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, f"{name} build failed:\n{log}"
        out[name] = exe
    return out


def run(exe, lines):
    env = dict(os.environ)
    env["UBSAN_OPTIONS"] = "halt_on_error=1 print_stacktrace=1"
    r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=300, env=env)
    report = r.stdout[-2000:] + r.stderr
    assert r.returncode == 0, report[-4000:]
    for mark in ("Sanitizer", "runtime error:"):
        assert mark not in report, report[-4000:]
    got = r.stdout.splitlines()
    assert got[-1] == "verify_units ok"
    return got[:-1]


def fields(line):
    return dict(tok.split("=") for tok in line.split())


def ints(line):
    return {k: int(v) for k, v in fields(line).items() if ":" not in v}


# ------------------------------------------------------------------------------------- pairing product
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_pairing_plan(binaries, kzgpot_mod, variant):
    ks = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 65535, MAX_PAIRS]
    prev = 0
    for k, line in zip(ks, run(binaries[variant], [f"pairing {k}" for k in ks])):
        p = ints(line)
        assert p["ok"] == 1 and p["k"] == k
        assert (p["lane_cells"], p["cell_bytes"], p["block"]) == (29, 112, 64)  # 29 cells of one Fq2 = 2 x 14 words
        # one lane per pair, whole Miller blocks, at least one
        assert p["stride"] % p["block"] == 0 and p["stride"] >= max(k, 1) and p["stride"] - p["block"] < max(k, 1)
        lanes_bytes = p["stride"] * p["lane_cells"] * p["cell_bytes"]
        assert p["lanes"] == 0 and p["final_cells"] % 256 == 0 and lanes_bytes <= p["final_cells"]
        assert p["final_cells"] + p["final_count"] * p["cell_bytes"] <= p["bytes"] == p["ws"]
        assert kzgpot_mod.pairing_workspace(k) == p["bytes"] >= prev
        prev = p["bytes"]
        # the tree: each level multiplies 256 live values per block, until one is left in lane 0
        levels = [tuple(int(x) for x in v.split(":")) for key, v in sorted(fields(line).items()) if key.startswith("level")]
        assert len(levels) == p["nlevels"] == (0 if k <= 1 else 1 if k <= 256 else 2)
        count, step = k, 1
        for c, s, blocks in levels:
            assert (c, s, blocks) == (count, step, -(-count // 256))
            assert (count - 1) * step < max(k, 1)  # the last live lane is a pair's lane
            count, step = blocks, step * 256
        assert count <= 1


def test_pairing_rejected(binaries, kzgpot_mod):
    got = run(binaries["asan_ubsan"], [f"pairing {MAX_PAIRS + 1}", f"pairing {1 << 40}"])
    assert [ints(l)["bytes"] for l in got] == [0, 0]
    assert kzgpot_mod.pairing_workspace(MAX_PAIRS + 1) == 0 and kzgpot_mod.pairing_workspace(1 << 63) == 0


# ------------------------------------------------------------------------------------- check / batch_check
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_check_plan(binaries, kzgpot_mod, variant):
    keys = [(n, c) for n in CHECK_NS for c in (0, 8, 16)]
    got = run(binaries[variant], [f"check {n} {c << 8}" for n, c in keys])
    prev = {}
    for (n, c), line in zip(keys, got):
        p = ints(line)
        assert p["ok"] == 1 and (p["n"], p["nbases"], p["c"]) == (n, 2 * n + 2, c)
        assert p["blocks"] == max(1, -(-n // 256))
        regions = [(p["bases"], 96 * p["nbases"]), (p["scalars"], 32 * p["nbases"]), (p["sums"], 2 * 32 * p["blocks"]),
                   (p["pairs_g1"], 2 * 96), (p["pairs_g2"], 2 * 192), (p["key2"], 8), (p["msm"], p["msm_bytes"]),
                   (p["pairing"], p["pairing_bytes"])]
        for (o0, s0), (o1, _) in zip(regions, regions[1:]):
            assert o0 % 256 == 0 and o0 + s0 <= o1, (n, c)
        assert regions[-1][0] + regions[-1][1] <= p["bytes"] == p["ws"]
        # the second MSM (the n proofs) runs in the first one's workspace
        assert 0 < p["msm_w_bytes"] <= p["msm_bytes"] == kzgpot_mod.msm_workspace(False, 2 * n + 2, c << 8)
        assert p["pairing_bytes"] == kzgpot_mod.pairing_workspace(2)
        assert kzgpot_mod.kzg_batch_check_workspace(n, c << 8) == p["bytes"] >= prev.get(c, 0)  # monotone in n
        prev[c] = p["bytes"]


def test_check_workspace_is_monotone(kzgpot_mod):
    sizes = [kzgpot_mod.kzg_batch_check_workspace(n) for n in list(range(0, 600)) + [1 << e for e in range(10, 25)] + [MAX_N]]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes)


def test_check_rejected(binaries, kzgpot_mod):
    cases = [(MAX_N + 1, 0), (1 << 40, 0), (5, 1), (5, 17 << 8), (5, 1 << 16), (5, 1 << 31), (MAX_N, 1 << 8)]
    got = run(binaries["plain"], [f"check {n} {flags}" for n, flags in cases])
    assert [ints(l)["bytes"] for l in got] == [0] * len(cases)
    for n, flags in cases:
        assert kzgpot_mod.kzg_batch_check_workspace(n, flags) == 0


# ------------------------------------------------------------------------------------- argument errors
def test_invalid_arguments_return_before_any_device_use(kzgpot_mod):
    """Every case is decided on the host: -100 with or without a GPU, and the outputs stay as they were."""
    from kzgpot import _lib

    lib = _lib.load()
    g1, g2, vk = b"\x00" * (96 * 4), b"\x00" * (192 * 4), b"\x00" * 576
    sc = b"\x01" * (32 * 4)
    out = ctypes.create_string_buffer(b"\xab" * 580, 580)
    fb = ctypes.c_int64(-1)

    prod = lib.kzgpot_pairing_product
    assert prod(None, g2, 4, out, ctypes.byref(fb)) == E_INVALID_ARG
    assert prod(g1, None, 4, out, ctypes.byref(fb)) == E_INVALID_ARG
    assert prod(g1, g2, MAX_PAIRS + 1, out, ctypes.byref(fb)) == E_INVALID_ARG
    dprod = lib.kzgpot_pairing_product_dev
    assert dprod(g1, g2, 4, out, None, out, None) == E_INVALID_ARG  # no workspace
    assert dprod(g1, g2, 4, out, out, None, None) == E_INVALID_ARG  # no key
    assert dprod(g1, g2, 4, None, out, out, None) == E_INVALID_ARG
    assert dprod(None, g2, 4, out, out, out, None) == E_INVALID_ARG
    assert dprod(g1, g2, MAX_PAIRS + 1, out, out, out, None) == E_INVALID_ARG

    batch = lib.kzgpot_kzg_batch_check
    good = [vk, g1, sc, sc, g1, sc, sc]
    for miss in (0, 1, 2, 3, 4, 6):  # every pointer but random_vs
        args = list(good)
        args[miss] = None
        assert batch(*args, 4, 0, ctypes.byref(fb)) == E_INVALID_ARG, miss
    assert batch(*good, MAX_N + 1, 0, ctypes.byref(fb)) == E_INVALID_ARG
    for flags in (1, 2, 17 << 8, 1 << 16, 1 << 31):
        assert batch(*good, 4, flags, ctypes.byref(fb)) == E_INVALID_ARG
    dbatch = lib.kzgpot_kzg_batch_check_dev
    assert dbatch(*good, 4, out, 0, None, out, None) == E_INVALID_ARG  # no workspace
    assert dbatch(*good, 4, out, 0, out, None, None) == E_INVALID_ARG  # no key
    assert dbatch(*good, 4, None, 0, out, out, None) == E_INVALID_ARG
    assert dbatch(*good, 4, out, 1, out, out, None) == E_INVALID_ARG
    one = lib.kzgpot_kzg_check
    assert one(None, g1, sc, sc, g1, None, ctypes.byref(fb)) == E_INVALID_ARG
    assert one(vk, None, sc, sc, g1, None, ctypes.byref(fb)) == E_INVALID_ARG
    assert one(vk, g1, None, sc, g1, sc, ctypes.byref(fb)) == E_INVALID_ARG
    assert one(vk, g1, sc, None, g1, sc, ctypes.byref(fb)) == E_INVALID_ARG
    assert one(vk, g1, sc, sc, None, sc, ctypes.byref(fb)) == E_INVALID_ARG
    assert out.raw == b"\xab" * 580 and fb.value == -1

    k = kzgpot_mod
    with pytest.raises(ValueError):
        k.pairing_product(g1, g2[:-1])
    with pytest.raises(ValueError):
        k.kzg_batch_check(vk[:-1], [g1[:96]], [1], [1], [g1[:96]], randomizers=[1])
    with pytest.raises(ValueError):
        k.kzg_batch_check(vk, [g1[:96]], [1, 2], [1], [g1[:96]], randomizers=[1])
