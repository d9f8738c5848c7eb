"""The multi-scalar multiplication below the whole call (csrc/msm_kernels.hip, DESIGN §10 "Tests").

tests/msm_cases.py holds crafted inputs that drive jac_madd's exceptional branches (doubling,
cancellation, going on after a cancellation) at each of the five places the schedule adds points;
tests/test_msm_model.py shows on the CPU that they reach those branches under every scatter order.
Here the same cases run on the device, in G1 and in G2:
  * the output record against ONE oracle scalar multiplication of the integer dot product, at the
    case's width, at the library's own width (the c = 8 cases) and from Montgomery base records;
  * the bit partials T_k, read back from the caller's workspace after a `_dev` call: slot
    final_base + k of the limb-major pool (row j of the pool is `cap` words long; pool, cap, rows,
    final_base and nseg come from msm_plan through tests/host_units/plan_units.cpp) carries the
    infinity mark the model's T_k asks for, zero coordinates when infinite, and otherwise canonical
    coordinates (limbs < 2^28, value < p) that leave Montgomery form (R = 2^392) as the oracle's
    affine [T_k]G — for G2 the c0 rows, then the c1 rows;
  * the workspace as scratch: a zero-filled, an all-ones and a stale workspace (left by a larger
    call of the same width) give the same record and the same final slots, and 4096 guard bytes
    behind the plan's size keep their pattern.

The widest window, c = 16, takes about 43 MB (G1) / 72 MB (G2) of workspace at n = 2, so its cases
run for both groups."""
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import kzgpot_oracle as O
import msm_cases as M
from test_gpu_lagrange import g1_points, g2_points
from test_gpu_msm import G2_K, INF1, INF2
from test_msm_model import msm_model
from test_plan_units import OUT, SRC, msm_line, parse

pytestmark = pytest.mark.gpu

R = O.R_ORDER
RINV = pow(1 << 392, -1, O.P)  # out of the device's Montgomery form
GUARD = 4096
GROUPS = pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
NAMES = [t.name for t in M.CASES]


# ------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def plan():
    """(g2, n, c) -> msm_plan's fields, from the plain build of the stand-alone plan program."""
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "plan_units_plain")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", SRC, "-o", exe], check=True)

    @functools.lru_cache(maxsize=None)
    def of(g2, n, c):
        r = subprocess.run([exe], input=msm_line(int(g2), n, c) + "\n", capture_output=True, text=True, timeout=60,
                           check=True)
        lines = r.stdout.splitlines()
        assert lines[-1] == "plan_units ok" and len(lines) == 2
        p = parse(lines[0])
        assert p["ok"] and p["rows"] == (57 if g2 else 29)
        return p
    return of


@pytest.fixture(scope="module")
def points(oracle_lib):
    """(g2, logs) -> the ark records of [k]G (k = 0: the point at infinity), one oracle call per distinct log."""
    cache = {}

    def of(g2, ks):
        new = sorted({k % R for k in ks} - {k for g, k in cache if g == g2})
        if new:
            recs, size = (g2_points(new), 192) if g2 else (g1_points(oracle_lib, new), 96)
            for i, k in enumerate(new):
                cache[g2, k] = recs[size * i: size * (i + 1)]
        return b"".join(cache[g2, k % R] for k in ks)
    return of


@pytest.fixture(scope="module")
def random_g1():
    """300 random logs and scalars (an infinite base among them)."""
    rng = random.Random(300)
    ks = [rng.randrange(1, R) for _ in range(300)]
    ks[17] = 0
    return ks, [rng.getrandbits(256) for _ in range(300)]


@pytest.fixture(scope="module")
def random_g2():
    """64 random scalars over the 64 G2 bases test_gpu_msm.py already multiplies out."""
    rng = random.Random(64)
    return list(G2_K), [rng.getrandbits(256) for _ in range(64)]


def ok(r):
    assert (r.ret, r.first_bad) == (0, -1)
    return r.out


def expected(points, g2, ks, scalars):
    d = sum(s * k for s, k in zip(scalars, ks)) % R
    return points(g2, [d]) if d else (INF2 if g2 else INF1)


# ------------------------------------------------------------------------------------- 1: the output record
@GROUPS
@pytest.mark.parametrize("name", NAMES)
def test_case_result(gpu, points, g2, name):
    t = M.BY_NAME[name]
    msm = gpu.g2_msm if g2 else gpu.g1_msm
    bases, want = points(g2, t.ks), expected(points, g2, t.ks, t.scalars)
    assert ok(msm(bases, t.scalars, window=t.c)) == want
    if t.c == 8:
        assert gpu.msm_window_bits(len(t.ks)) == 8
        assert ok(msm(bases, t.scalars, window=0)) == want
    mont = gpu.deserialize_unchecked(bases, g2=g2)
    assert mont.ret == 0
    assert ok(msm(mont.out, t.scalars, mont=True, window=t.c)) == want


# ------------------------------------------------------------------------------------- 2: the bit partials
def run_dev(gpu, plan, g2, bases, scalars, c, work=None, fill=None):
    """One `_dev` call with an explicit width on a workspace of the plan's bytes + GUARD that the
    test owns (filled with `fill` unless `work` is given) -> (record, the nseg final slots as a
    (rows, nseg) uint32 array, the guard bytes, the plan)."""
    import torch
    from kzgpot import device as D

    n = len(scalars)
    p = plan(g2, n, c)
    assert p["bytes"] == gpu.msm_workspace(g2, n, c << 8)
    dev = torch.device("cuda:0")
    if work is None:
        work = torch.full((p["bytes"] + GUARD,), fill, dtype=torch.uint8, device=dev)
    assert work.numel() == p["bytes"] + GUARD
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    out = torch.full((192 if g2 else 96,), 0xAB, dtype=torch.uint8, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    D.msm_dev(g2, to_dev(bases), to_dev(b"".join(s.to_bytes(32, "little") for s in scalars)), out, key, window=c,
              work=work)
    torch.cuda.synchronize()
    assert D.read_key(key) == (1 << 64) - 1
    rows, cap, fb, nseg = p["rows"], p["cap"], p["final_base"], p["nseg"]
    assert fb + nseg <= cap and p["pool"] + rows * cap * 4 <= p["bytes"]
    pool = work[p["pool"]: p["pool"] + rows * cap * 4].view(torch.int32).view(rows, cap)
    slots = pool[:, fb: fb + nseg].contiguous().cpu().numpy().view(np.uint32)
    return bytes(out.cpu().numpy()), slots, bytes(work[p["bytes"]:].cpu().numpy()), p


def check_partials(points, g2, slots, tk, where):
    rows, nseg = slots.shape
    ncoord = 4 if g2 else 2  # x (c0, c1), y (c0, c1): 14 limb rows each, then the infinity row
    assert rows == 14 * ncoord + 1 and nseg == len(tk)
    finite = sorted({v for v in tk if v})
    recs = points(g2, finite)
    affine = {}
    for i, v in enumerate(finite):
        if g2:
            st, (x, y, inf) = O.ark_g2_deserialize_uncompressed(recs[192 * i: 192 * (i + 1)], subgroup_check=False)
            affine[v] = [x[0], x[1], y[0], y[1]]
        else:
            st, (x, y, inf) = O.ark_g1_deserialize_uncompressed(recs[96 * i: 96 * (i + 1)], subgroup_check=False)
            affine[v] = [x, y]
        assert st == 0 and not inf
    for k, v in enumerate(tk):
        col = [int(w) for w in slots[:, k]]
        assert col[-1] == (0 if v else 1), (where, k, col[-1])
        if not v:
            assert not any(col[:-1]), (where, k)
            continue
        for j, want in enumerate(affine[v]):
            limbs = col[14 * j: 14 * j + 14]
            assert max(limbs) < 1 << 28, (where, k, j)
            val = sum(w << (28 * i) for i, w in enumerate(limbs))
            assert val < O.P, (where, k, j)
            assert val * RINV % O.P == want, (where, k, j)


@GROUPS
@pytest.mark.parametrize("name", NAMES)
def test_case_partials(gpu, plan, points, g2, name):
    t = M.BY_NAME[name]
    tk = []
    assert msm_model(t.ks, t.scalars, t.c, partials=tk)[0] == M.dot(t)
    assert sum(1 for v in tk if v) <= 8  # a G2 point from the oracle costs about 14 ms
    out, slots, guard, _ = run_dev(gpu, plan, g2, points(g2, t.ks), t.scalars, t.c, fill=0)
    check_partials(points, g2, slots, tk, name)
    assert out == expected(points, g2, t.ks, t.scalars) and guard == bytes(GUARD)


@pytest.mark.parametrize("c", [1, 5, 8, 13, 16])
def test_random_partials(gpu, plan, points, random_g1, c):
    ks, s = random_g1
    tk = []
    msm_model(ks, s, c, partials=tk)
    out, slots, guard, _ = run_dev(gpu, plan, False, points(False, ks), s, c, fill=0)
    check_partials(points, False, slots, tk, c)
    assert out == expected(points, False, ks, s) and guard == bytes(GUARD)


# ------------------------------------------------------------------------------------- 3: the workspace is scratch
def three_workspaces(gpu, plan, points, g2, ks, scalars, c, big_ks):
    """The same call on a zero-filled, an all-ones and a stale workspace: one record, one set of
    final slots, the guard bytes untouched."""
    import torch

    bases = points(g2, ks)
    runs = [run_dev(gpu, plan, g2, bases, scalars, c, fill=fill) for fill in (0x00, 0xFF)]
    assert [r[2] for r in runs] == [bytes(GUARD), b"\xff" * GUARD]
    # stale: what a larger call of the same width left (all scalars equal: every level runs full)
    p = runs[0][3]
    big = plan(g2, len(big_ks), c)
    assert big["bytes"] >= p["bytes"] + GUARD
    one = random.Random(c).getrandbits(256)
    stale = torch.empty(big["bytes"] + GUARD, dtype=torch.uint8, device="cuda:0")
    out_big, _, _, _ = run_dev(gpu, plan, g2, points(g2, big_ks), [one] * len(big_ks), c, work=stale)
    assert out_big == expected(points, g2, big_ks, [one] * len(big_ks))
    work = stale[: p["bytes"] + GUARD]
    work[p["bytes"]:] = 0xA5
    assert int(work[: p["bytes"]].max()) > 0  # not cleared
    runs.append(run_dev(gpu, plan, g2, bases, scalars, c, work=work))
    assert runs[2][2] == b"\xa5" * GUARD
    want = expected(points, g2, ks, scalars)
    for out, slots, _, _ in runs:
        assert out == want
        assert slots.tobytes() == runs[0][1].tobytes()
    return runs[0][1]


@pytest.fixture(scope="module")
def big_g1():
    rng = random.Random(2047)
    return [rng.randrange(1, R) for _ in range(2047)]


@pytest.mark.parametrize("name", ["random", "bucket1 cancel", "bits1 cancel", "final go on after cancel"])
def test_workspace_is_scratch_g1(gpu, plan, points, random_g1, big_g1, name):
    ks, s = random_g1 if name == "random" else (M.BY_NAME[name].ks, M.BY_NAME[name].scalars)
    slots = three_workspaces(gpu, plan, points, False, ks, s, 8, big_g1)
    tk = []
    msm_model(ks, s, 8, partials=tk)
    check_partials(points, False, slots, tk, name)


def test_workspace_is_scratch_g2(gpu, plan, points, random_g2):
    ks, s = random_g2
    three_workspaces(gpu, plan, points, True, ks, s, 8, (list(G2_K) * 32)[:2047])
