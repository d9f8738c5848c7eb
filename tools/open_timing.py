"""Timing record of the polynomial division (kzgpot_fr_poly_divide_dev, csrc/poly_kernels.hip) and
of KZG10 open (kzgpot_g1_kzg_open_dev, csrc/open.hip) on device-resident data.

    python3 tools/open_timing.py [--divide 20,24] [--open-log2 20] > profiles/open_timing.json

A record, not a gate: nothing comparable exists to measure against, no threshold is fixed in
advance and no speed-up over a CPU is claimed. Device-resident, timed by events, best of two
launches after a warm-up, next to the shader clock (k_clock_probe). Three things in one run:

  * the division at each size, with the library's tile and with every tile override, against a
    device-to-device copy that moves the same bytes: the kernels read every coefficient twice (the
    up pass and the down pass both stage the tile) and write the quotient once, 96 B per
    coefficient (the upper levels add 96 / S of that), so the copy is 48 n bytes read and 48 n
    bytes written;
  * open at 2^open_log2 coefficients, not hiding, over synthetic subgroup points;
  * the MSM alone over the same n - 1 bases with uniform random 256-bit scalars: the part open
    cannot avoid. open - MSM is what the division and the staging copy of the bases cost."""
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


def timed(dev, fn, launches):
    """best (ms, MHz) of `launches` runs of fn after one warm-up. The clock probe's two readings
    bracket the launch; for launches of a few milliseconds their difference is noise (it has come
    out negative, and above 10 GHz), so the clock is reported only for launches of 10 ms and more."""
    fn()
    torch.cuda.synchronize()
    rows = []
    for _ in range(launches):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        c0 = D.clock_probe(dev)
        ev[0].record()
        fn()
        ev[1].record()
        c1 = D.clock_probe(dev)
        torch.cuda.synchronize()
        clk = D.clock_mhz(c0, c1)
        rows.append((ev[0].elapsed_time(ev[1]), clk["mean"] if clk else None))
    ms, mhz = min(rows, key=lambda r: r[0])
    return {"ms_per_launch": [round(r[0], 4) for r in rows], "best_ms": round(ms, 4),
            "shader_mhz": round(mhz) if mhz and ms >= 10.0 else None}


def random_bytes(rng, n, dev):
    words = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64, endpoint=False)
    return torch.from_numpy(words.view(np.uint8).reshape(-1)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--divide", default="20,24")
    ap.add_argument("--open-log2", type=int, default=20)
    ap.add_argument("--launches", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2027)
    z = int.from_bytes(rng.bytes(32), "little")
    res = {"tool": "tools/open_timing.py", "device": torch.cuda.get_device_name(0), "version": kzgpot.version(),
           "bytes_per_coefficient": {"read": 64, "written": 32}, "rows": []}

    def add(row):
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    for lg in [int(e) for e in a.divide.split(",") if e]:
        n = 1 << lg
        coeffs = random_bytes(rng, n, dev)
        quot = torch.empty(32 * (n - 1), dtype=torch.uint8, device=dev)
        value = torch.empty(32, dtype=torch.uint8, device=dev)
        src, dst = (torch.empty(48 * n, dtype=torch.uint8, device=dev) for _ in range(2))
        src.zero_()
        copy = timed(dev, lambda: dst.copy_(src), a.launches)
        add(dict(copy, what="d2d copy", n=n, bytes_moved=96 * n, gb_per_s=round(96 * n / copy["best_ms"] * 1e-6, 1)))
        first = None
        for tile in (0, 8, 9, 10, 11, 12):
            work = torch.empty(kzgpot.fr_poly_workspace(n, tile << 16), dtype=torch.uint8, device=dev)
            row = timed(dev, lambda: D.fr_poly_divide_dev(coeffs, z, quot, value, tile=tile, work=work), a.launches)
            ev = timed(dev, lambda: D.fr_poly_divide_dev(coeffs, z, None, value, tile=tile, work=work), a.launches)
            got = bytes(value.cpu().numpy()) + bytes(quot[:64].cpu().numpy())
            first = first or got
            add(dict(row, what="divide", n=n, tile=tile, bytes_moved=96 * n,
                     gb_per_s=round(96 * n / row["best_ms"] * 1e-6, 1),
                     over_copy=round(row["best_ms"] / copy["best_ms"], 2), evaluate_only_ms=ev["best_ms"],
                     same_as_library_tile=got == first))
        del coeffs, quot, src, dst

    if a.open_log2:
        n = 1 << a.open_log2
        _, ark = D.synth("g1", 5, 0, n - 1, dev)
        coeffs = random_bytes(rng, n, dev)
        out = torch.empty(160, dtype=torch.uint8, device=dev)
        key = torch.empty(1, dtype=torch.int64, device=dev)
        work = torch.empty(kzgpot.kzg_open_workspace(n), dtype=torch.uint8, device=dev)
        opn = timed(dev, lambda: D.g1_kzg_open_dev(ark, coeffs, z, out, key, work=work), a.launches)
        add(dict(opn, what="open", n=n, hiding=False, workspace_bytes=int(work.numel()),
                 all_accepted=D.read_key(key) == (1 << 64) - 1, out=bytes(out.cpu().numpy()).hex()))
        scal = random_bytes(rng, n - 1, dev)
        point = torch.empty(96, dtype=torch.uint8, device=dev)
        mwork = work[: kzgpot.msm_workspace(False, n - 1)]
        msm = timed(dev, lambda: D.g1_msm_dev(ark, scal, point, key, work=mwork), a.launches)
        add(dict(msm, what="msm", n=n - 1, scalars="random", window_bits=kzgpot.msm_window_bits(n - 1)))
        stage = timed(dev, lambda: work[: 96 * (n - 1)].copy_(ark), a.launches)
        add(dict(stage, what="staging copy of the bases", n=n - 1, bytes=96 * (n - 1)))
        res["open_minus_msm_ms"] = round(opn["best_ms"] - msm["best_ms"], 4)
        res["open_minus_msm_over_msm"] = round((opn["best_ms"] - msm["best_ms"]) / msm["best_ms"], 4)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
