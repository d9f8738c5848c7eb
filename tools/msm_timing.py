"""Timing record of the multi-scalar multiplication (kzgpot_g1_msm_dev / kzgpot_g2_msm_dev,
csrc/msm_kernels.hip) on device-resident subgroup points from the synthetic generator.

    python3 tools/msm_timing.py [--g1 16,20,22] [--g2 16,20] [--equal-log2 20] > profiles/msm_timing.json

A record, not a gate: nobody has measured an MSM on this hardware and the repository has nothing
comparable to measure against, so no speed-up over a CPU is claimed. Scalars are uniform random
256-bit integers, plus one row with all scalars equal (every window's points in one bucket).
Device-resident, timed by events, best of two launches after a warm-up, next to the shader clock
(k_clock_probe). Each row carries a ceiling derived from DESIGN.md §9's measured primitive peaks
at 2,338 MHz, scaled by the measured clock, and the fraction of it reached:

    (n W + 256 x 2^(c-1)) mixed additions at 0.136 ns (G1) / 0.390 ns (G2) chip-wide
    + one 5.1 ns inversion per normalised partial sum

with W = ceil(256 / c). The partial sums are counted from the scalars' own digit histogram: at
every level a bucket of x entries gives floor(x / 64) full chunks and a remainder, and a chunk of
two or more entries is normalised (a chunk of one is copied); every chunk of the bit partials'
static lists is counted as normalised; plus the final one. The ceiling ignores the gathers, the
count / scan / scatter launches and the 256 doublings of the one-lane final ladder, whose time is
reported on its own (`final_ladder_ms`: the same call at n = 1, which is that ladder and the
launches of an empty schedule)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "kzg-setup-powersoftau_amd"))
import kzgpot  # noqa: E402
from kzgpot import device as D  # noqa: E402

PEAK_MHZ = 2338.0
MADD_NS = {False: 0.136, True: 0.390}
INV_NS = 5.1
L = 64


def digits(words: np.ndarray, j: int, c: int) -> np.ndarray:
    """Digit j (c bits) of n little-endian 256-bit scalars given as an (n, 4) uint64 array."""
    bit = j * c
    w, sh = bit // 64, bit % 64
    v = words[:, w] >> np.uint64(sh)
    if sh + c > 64 and w + 1 < 4:
        v = v | (words[:, w + 1] << np.uint64(64 - sh))
    return (v & np.uint64((1 << c) - 1)).astype(np.int64)


def normalised_partials(words: np.ndarray, c: int) -> int:
    nwin, total = -(-256 // c), 0
    for j in range(nwin):
        cnt = np.bincount(digits(words, j, c), minlength=1 << c)[1:]
        while cnt.max(initial=0) > 1:
            total += int((cnt // L).sum() + ((cnt % L) >= 2).sum())
            cnt = -(-cnt // L)
    seg = 1 << (c - 1)
    while True:
        seg = -(-seg // L)
        total += nwin * c * seg
        if seg == 1:
            break
    return total + 1


def time_msm(g2: bool, n: int, bases: torch.Tensor, words: np.ndarray, launches: int, label: str):
    dev = bases.device
    rec = 192 if g2 else 96
    scal = torch.from_numpy(words.view(np.uint8).reshape(-1)).to(dev)
    out = torch.empty(rec, dtype=torch.uint8, device=dev)
    key = torch.empty(1, dtype=torch.int64, device=dev)
    work = torch.empty(kzgpot.msm_workspace(g2, n), dtype=torch.uint8, device=dev)
    x = bases[: n * rec]
    D.msm_dev(g2, x, scal, out, key, work=work)  # warm-up
    torch.cuda.synchronize()
    rows = []
    for _ in range(launches):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        c0 = D.clock_probe(dev)
        ev[0].record()
        D.msm_dev(g2, x, scal, out, key, work=work)
        ev[1].record()
        c1 = D.clock_probe(dev)
        torch.cuda.synchronize()
        clk = D.clock_mhz(c0, c1)
        rows.append((ev[0].elapsed_time(ev[1]), clk["mean"] if clk else None))
    ms, mhz = min(rows, key=lambda r: r[0])
    c = kzgpot.msm_window_bits(n)
    nwin = -(-256 // c)
    madds = n * nwin + 256 * (1 << (c - 1))
    partials = normalised_partials(words, c)
    ceil_ms = (madds * MADD_NS[g2] + partials * INV_NS) * 1e-6 * (PEAK_MHZ / (mhz or PEAK_MHZ))
    return {"group": "g2" if g2 else "g1", "n": n, "scalars": label, "window_bits": c, "windows": nwin,
            "ms_per_launch": [round(r[0], 3) for r in rows], "best_ms": round(ms, 3),
            "shader_mhz": round(mhz) if mhz else None, "points_per_s": n / ms * 1e3,
            "mixed_additions": madds, "normalised_partials": partials, "ceiling_ms": round(ceil_ms, 3),
            "fraction_of_ceiling": round(ceil_ms / ms, 3), "workspace_bytes": int(work.numel()),
            "all_accepted": D.read_key(key) == (1 << 64) - 1, "out": bytes(out.cpu().numpy()).hex()}


def random_words(rng, n):
    return rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64, endpoint=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1", default="16,20,22")
    ap.add_argument("--g2", default="16,20")
    ap.add_argument("--equal-log2", type=int, default=20, help="the all-equal-scalar G1 row; 0: skip")
    ap.add_argument("--launches", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2026)
    res = {"tool": "tools/msm_timing.py", "device": torch.cuda.get_device_name(0), "version": kzgpot.version(),
           "ceiling": {"madd_ns_at_2338MHz": {"g1": MADD_NS[False], "g2": MADD_NS[True]}, "inversion_ns": INV_NS,
                       "chunk": L}, "rows": []}

    def add(row):
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    for g2, logs in ((False, a.g1), (True, a.g2)):
        logs = [int(e) for e in logs.split(",") if e]
        if not logs:
            continue
        top = max(logs + ([a.equal_log2] if not g2 else []))
        _, ark = D.synth("g2" if g2 else "g1", 5, 0, 1 << top, dev)
        add(dict(time_msm(g2, 1, ark, random_words(rng, 1), a.launches, "random"), role="final_ladder_ms"))
        for lg in logs:
            add(time_msm(g2, 1 << lg, ark, random_words(rng, 1 << lg), a.launches, "random"))
        if not g2 and a.equal_log2:
            n = 1 << a.equal_log2
            add(time_msm(g2, n, ark, np.repeat(random_words(rng, 1), n, axis=0), a.launches, "all equal"))
        del ark
        torch.cuda.empty_cache()
    rnd = {(r["group"], r["n"]): r for r in res["rows"] if r["scalars"] == "random"}
    for r in res["rows"]:
        if r["scalars"] == "all equal":
            res["all_equal_over_random"] = {"n": r["n"], "ratio": round(r["best_ms"] / rnd[(r["group"], r["n"])]["best_ms"], 3)}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
