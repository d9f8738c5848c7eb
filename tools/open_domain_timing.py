"""Timing record of the NTT over Fr (kzgpot_fr_ntt_dev, csrc/ntt_kernels.hip) and of the amortized
KZG10 openings over a domain (kzgpot_g1/g2_open_domain_dev, csrc/domain.hip) on device-resident data.

    python3 tools/open_domain_timing.py [--ntt 16,20,22,24] [--g1 16,20] [--g2 16] > profiles/open_domain_timing.json

A record, not a gate: nothing comparable exists to measure against, no threshold is fixed in
advance and no speed-up over a CPU is claimed. Device-resident, timed by events, best of two
launches after a warm-up, next to the shader clock (k_clock_probe). In one run:

  * the NTT at each size with every supported tile and last with the library's (tile 0), out of
    place, against a device-to-device copy of the same 32 m bytes; a pass reads and writes every
    element once, so `over_copy_per_pass` = time / (passes x copy time) is how far a pass is from
    moving its bytes. The launches are sub-millisecond to a few milliseconds, so 50 untimed launches
    at each size bring the clock up before the first timed one. The library's tile is the one that
    measures fastest at 2^22;
  * the opening at 2^exp points over synthetic subgroup points: the whole call, the table
    separately, and the two group transforms the call cannot avoid, kzgpot_g1_fft_dev inverse at
    exp + 1 and forward at exp over the same kind of points. call - transforms is what the two
    NTTs, the per-point pass and the gather cost less the scale pass the call drops: the per-point
    pass is 2n scalar multiplications, `derived_per_point_pass_over_butterflies` of the
    n (exp + 1) + n exp / 2 butterflies of the two transforms (one scalar multiplication each), and
    the measured inverse transform contains a scale pass of the same 2n scalar multiplications, so
    by the operation count the two cancel and the remainder is the field side alone;
  * one kzgpot_g1_kzg_open_dev at n = 2^exp coefficients, and n times that: the cost of the n
    openings one point at a time."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "kzg-setup-powersoftau_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzgpot  # noqa: E402
from kzgpot import device as D  # noqa: E402
from open_timing import random_bytes, timed  # noqa: E402

TILES = (8, 9, 10, 11)


def passes(exp, tile):
    return max(1, -(-exp // tile))


def ntt_rows(dev, rng, exps, launches, add):
    for lg in exps:
        m = 1 << lg
        x = random_bytes(rng, m, dev)
        out, dst = (torch.empty(32 * m, dtype=torch.uint8, device=dev) for _ in range(2))
        copy = timed(dev, lambda: dst.copy_(x), launches)
        add(dict(copy, what="d2d copy", m=m, bytes=32 * m, gb_per_s=round(64 * m / copy["best_ms"] * 1e-6, 1)))
        warm = torch.empty(kzgpot.fr_ntt_workspace(lg, 0), dtype=torch.uint8, device=dev)
        for _ in range(50):
            D.fr_ntt_dev(x, lg, out, work=warm)
        torch.cuda.synchronize()
        first = None
        for tile in TILES + (0,):
            work = torch.empty(kzgpot.fr_ntt_workspace(lg, tile << 16), dtype=torch.uint8, device=dev)
            row = timed(dev, lambda: D.fr_ntt_dev(x, lg, out, tile=tile, work=work), launches)
            got = bytes(out[:64].cpu().numpy()) + bytes(out[-64:].cpu().numpy())
            first = first or got  # tile 8's: every tile must agree with it
            t = tile or kzgpot.NTT_DEFAULT_TILE
            add(dict(row, what="ntt", m=m, exp=lg, tile=tile, passes=passes(lg, t),
                     over_copy_per_pass=round(row["best_ms"] / (passes(lg, t) * copy["best_ms"]), 2),
                     ns_per_butterfly=round(row["best_ms"] * 1e6 / (m / 2 * max(1, lg)), 3),
                     same_as_first_tile=got == first))
        del x, out, dst


def open_rows(dev, rng, g2, exp, launches, add):
    kind, rec = ("g2", 192) if g2 else ("g1", 96)
    n = 1 << exp
    _, powers = D.synth(kind, 7, 0, n, dev)
    coeffs = random_bytes(rng, n, dev)
    key = torch.empty(1, dtype=torch.int64, device=dev)
    table = torch.empty(2 * n * rec, dtype=torch.uint8, device=dev)
    twork = torch.empty(kzgpot.open_domain_table_workspace(g2, exp), dtype=torch.uint8, device=dev)
    tab = timed(dev, lambda: D.open_domain_table_dev(g2, powers, exp, table, key, work=twork), launches)
    add(dict(tab, what="table", group=kind, exp=exp, workspace_bytes=int(twork.numel()),
             all_accepted=D.read_key(key) == (1 << 64) - 1))
    del twork
    proofs = torch.empty(n * rec, dtype=torch.uint8, device=dev)
    values = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    work = torch.empty(kzgpot.open_domain_workspace(g2, exp), dtype=torch.uint8, device=dev)
    call = timed(dev, lambda: D.open_domain_dev(g2, table, coeffs, exp, proofs, values, key, work=work), launches)
    add(dict(call, what="open_domain", group=kind, exp=exp, workspace_bytes=int(work.numel()),
             all_accepted=D.read_key(key) == (1 << 64) - 1, proofs_head=bytes(proofs[:rec].cpu().numpy()).hex()))
    # the two transforms the call cannot avoid, over the table (2n points) and the proofs (n points)
    fwork = work[: kzgpot.group_fft_workspace(g2, exp + 1)]
    wide = timed(dev, lambda: D.group_fft_dev(g2, table, exp + 1, table, key, inverse=True, work=fwork), launches)
    add(dict(wide, what="group fft inverse", group=kind, exp=exp + 1))
    outp = timed(dev, lambda: D.group_fft_dev(g2, proofs, exp, proofs, key, inverse=False, work=fwork), launches)
    add(dict(outp, what="group fft forward", group=kind, exp=exp))
    both = wide["best_ms"] + outp["best_ms"]
    butterflies = n * (exp + 1) + n * exp / 2
    row = {"what": "open_domain minus transforms", "group": kind, "exp": exp,
           "call_ms": call["best_ms"], "transforms_ms": round(both, 4), "rest_ms": round(call["best_ms"] - both, 4),
           "rest_over_transforms": round((call["best_ms"] - both) / both, 4),
           # 2n scalar multiplications, in the call and not in the transforms; the dropped scale pass
           # is as many, in the transforms and not in the call
           "derived_per_point_pass_over_butterflies": round(2 * n / butterflies, 4)}
    if not g2:
        z = int.from_bytes(rng.bytes(32), "little")
        out = torch.empty(160, dtype=torch.uint8, device=dev)
        owork = torch.empty(kzgpot.kzg_open_workspace(n), dtype=torch.uint8, device=dev)
        one = timed(dev, lambda: D.g1_kzg_open_dev(powers, coeffs, z, out, key, work=owork), launches)
        add(dict(one, what="kzg_open at one point", n=n))
        row.update(one_open_ms=one["best_ms"], n_opens_s=round(one["best_ms"] * n * 1e-3, 1),
                   n_opens_over_call=round(one["best_ms"] * n / call["best_ms"], 1))
    add(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ntt", default="16,20,22,24")
    ap.add_argument("--g1", default="16,20")
    ap.add_argument("--g2", default="16")
    ap.add_argument("--launches", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2028)
    res = {"tool": "tools/open_domain_timing.py", "device": torch.cuda.get_device_name(0), "version": kzgpot.version(),
           "library_tile": kzgpot.NTT_DEFAULT_TILE, "rows": []}

    def add(row):
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    exps = lambda s: [int(e) for e in s.split(",") if e]  # noqa: E731
    ntt_rows(dev, rng, exps(a.ntt), a.launches, add)
    for g2, arg in ((False, a.g1), (True, a.g2)):
        for exp in exps(arg):
            open_rows(dev, rng, g2, exp, a.launches, add)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
