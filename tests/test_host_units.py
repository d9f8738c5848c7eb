"""The library's host machinery (csrc/host_rt.hpp, csrc/chunk_plan.hpp: threads, Watermark,
OrderedWorker, ShardCursor, HostBuf / Releaser, TempOutput, ChunkPlan) checked by a stand-alone
program with its own main (tests/host_units/host_units.cpp), built with g++ three ways: plain,
under the thread sanitizer, and under the address + undefined-behaviour sanitizers. No GPU, no HIP
header, nothing preloaded: each binary runs as a child process and must exit 0 without a
sanitizer report."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "host_units", "host_units.cpp")
OUT = os.path.join(ROOT, "tests", "host_units", "build")
VARIANTS = {"plain": [], "tsan": ["-fsanitize=thread"], "asan_ubsan": ["-fsanitize=address,undefined"]}


@pytest.fixture(scope="module")
def binaries():
    """The three builds, compiled side by side."""
    os.makedirs(OUT, exist_ok=True)
    procs = {}
    for name, flags in VARIANTS.items():
        exe = os.path.join(OUT, "host_units_" + name)
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wall", "-DKZGPOT_TEST_HOOKS", *flags, SRC, "-o", exe, "-ldl"]
        procs[name] = (exe, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    out = {}
    for name, (exe, p) in procs.items():
        log = p.communicate()[0]
        assert p.returncode == 0, f"{name} build failed:\n{log}"
        out[name] = exe
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_host_units(binaries, variant, tmp_path):
    env = dict(os.environ)
    # a sanitizer finding ends the run with a non-zero exit code instead of only a report
    env["TSAN_OPTIONS"] = "halt_on_error=1 exitcode=66"
    env["UBSAN_OPTIONS"] = "halt_on_error=1 print_stacktrace=1"
    r = subprocess.run([binaries[variant], str(tmp_path)], capture_output=True, text=True, timeout=60, env=env)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report
    assert "host_units ok" in r.stdout
    for mark in ("Sanitizer", "runtime error:", "CHECK failed"):
        assert mark not in report, report
    assert not list(tmp_path.iterdir())
