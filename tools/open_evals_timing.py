"""Timing record of the evaluation-form path (csrc/eval_kernels.hip, csrc/evals.hip) on device-resident
data: the batch inversion, the division in evaluation form and KZG10 open from evaluations.

    python3 tools/open_evals_timing.py [--exps 16,20] [--reps 5] [--out profiles/open_evals_timing.json]

A record, not a gate: the reference has nothing comparable, no threshold is fixed in advance and no
speed-up over a CPU is claimed; a ratio is formed only between rows of the same run. Device events,
one warm-up launch, `reps` timed launches reported as min / median / max, next to the shader clock
(k_clock_probe; for launches under 10 ms its two readings do not bracket enough time and it is not
reported). At each exp, in one process:

  1 the Fr part alone: kzgpot_fr_evals_divide_dev at every tile and the library's, with the
    quotient and evaluate-only, z off the domain and on it, against a device-to-device copy of the
    bytes its passes move, counted from the plan: k_eval_inv reads the evaluations and writes the
    inverted differences (32 n + 32 n), k_eval_quot reads both and writes the quotient (64 n + 32 n),
    160 n bytes in all, so the copy is 80 n bytes read and 80 n written. kzgpot_fr_batch_inverse_dev
    (32 n read, 32 n written) against a copy of 32 n bytes;
  2 kzgpot_g1_kzg_open_evals_dev against kzgpot_g1_msm_dev alone over the same bases and the same
    quotient scalars: open - MSM is what the Fr part costs inside the call;
  3 kzgpot_g1_kzg_open_evals_dev against the route without it for the same input: the inverse
    kzgpot_fr_ntt_dev, then kzgpot_g1_kzg_open_dev over the monomial powers (the same synthetic
    points stand in for both bases: only the time is compared).

The share of the Fr part that the one inversion per tile accounts for is not separated by this
tool: it would need a build of the kernels without the inversion."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "kzg-setup-powersoftau_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kzgpot  # noqa: E402
from kzgpot import device as D  # noqa: E402
from open_timing import random_bytes  # noqa: E402

R = kzgpot.R_ORDER
TILES = (8, 9, 10, 11, 12)


def timed(dev, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms, mhz = [], []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        c0 = D.clock_probe(dev)
        ev[0].record()
        fn()
        ev[1].record()
        c1 = D.clock_probe(dev)
        torch.cuda.synchronize()
        clk = D.clock_mhz(c0, c1)
        ms.append(ev[0].elapsed_time(ev[1]))
        mhz.append(clk["mean"] if clk else None)
    best = min(range(reps), key=lambda i: ms[i])
    return {"min_ms": round(min(ms), 4), "median_ms": round(statistics.median(ms), 4), "max_ms": round(max(ms), 4),
            "reps": reps, "shader_mhz_at_min": round(mhz[best]) if mhz[best] and mhz[best] > 0 and ms[best] >= 10.0 else None}


def fr_rows(dev, rng, exp, reps, add):
    n = 1 << exp
    evals = random_bytes(rng, n, dev)
    quot = torch.empty(32 * n, dtype=torch.uint8, device=dev)
    value = torch.empty(32, dtype=torch.uint8, device=dev)
    z_off = int.from_bytes(rng.bytes(32), "little")
    z_on = pow(kzgpot.fr_domain_root(exp), n // 3, R)
    src, dst = (torch.zeros(80 * n, dtype=torch.uint8, device=dev) for _ in range(2))
    copy = timed(dev, lambda: dst.copy_(src), reps)
    add(dict(copy, what="d2d copy of the division's bytes", exp=exp, bytes_moved=160 * n,
             gb_per_s=round(160 * n / copy["min_ms"] * 1e-6, 1)))
    small = timed(dev, lambda: dst[: 32 * n].copy_(src[: 32 * n]), reps)
    add(dict(small, what="d2d copy of the inversion's bytes", exp=exp, bytes_moved=64 * n,
             gb_per_s=round(64 * n / small["min_ms"] * 1e-6, 1)))
    first = {}
    for tile in TILES + (0,):
        work = torch.empty(kzgpot.fr_evals_workspace(exp, tile << 16), dtype=torch.uint8, device=dev)
        for where, z in (("off the domain", z_off), ("on the domain", z_on)):
            row = timed(dev, lambda: D.fr_evals_divide_dev(evals, exp, z, quot, value, tile=tile, work=work), reps)
            got = bytes(value.cpu().numpy()) + bytes(quot[:64].cpu().numpy()) + bytes(quot[-64:].cpu().numpy())
            ev = timed(dev, lambda: D.fr_evals_divide_dev(evals, exp, z, None, value, tile=tile, work=work), reps)
            add(dict(row, what="evals divide", exp=exp, tile=tile, z=where, bytes_moved=160 * n,
                     gb_per_s=round(160 * n / row["min_ms"] * 1e-6, 1), over_copy=round(row["min_ms"] / copy["min_ms"], 2),
                     evaluate_only_min_ms=ev["min_ms"], same_as_first_tile=got == first.setdefault(where, got)))
        inv = timed(dev, lambda: D.fr_batch_inverse_dev(evals, quot, tile=tile), reps)
        add(dict(inv, what="batch inverse", exp=exp, tile=tile, bytes_moved=64 * n,
                 gb_per_s=round(64 * n / inv["min_ms"] * 1e-6, 1), over_copy=round(inv["min_ms"] / small["min_ms"], 2),
                 inversion_share="not measured"))
    del src, dst


def open_rows(dev, rng, exp, reps, add):
    n = 1 << exp
    _, bases = D.synth("g1", 9, 0, n, dev)
    evals = random_bytes(rng, n, dev)
    z = int.from_bytes(rng.bytes(32), "little")
    key = torch.empty(1, dtype=torch.int64, device=dev)
    out = torch.empty(160, dtype=torch.uint8, device=dev)
    work = torch.empty(kzgpot.kzg_open_evals_workspace(exp), dtype=torch.uint8, device=dev)
    opn = timed(dev, lambda: D.g1_kzg_open_evals_dev(bases, evals, exp, z, out, key, work=work), reps)
    add(dict(opn, what="open from evaluations", exp=exp, workspace_bytes=int(work.numel()),
             all_accepted=D.read_key(key) == (1 << 64) - 1, out=bytes(out[:128].cpu().numpy()).hex()))
    # the MSM alone: the same bases, the same quotient
    quot = torch.empty(32 * n, dtype=torch.uint8, device=dev)
    fwork = work[: kzgpot.fr_evals_workspace(exp)]
    fr = timed(dev, lambda: D.fr_evals_divide_dev(evals, exp, z, quot, out[128:], work=fwork), reps)
    add(dict(fr, what="evals divide (the open's Fr part)", exp=exp))
    point = torch.empty(96, dtype=torch.uint8, device=dev)
    mwork = torch.empty(kzgpot.msm_workspace(False, n), dtype=torch.uint8, device=dev)
    msm = timed(dev, lambda: D.g1_msm_dev(bases, quot, point, key, work=mwork), reps)
    add(dict(msm, what="msm over the same bases and quotient", exp=exp, window_bits=kzgpot.msm_window_bits(n),
             same_point_as_open=bytes(point.cpu().numpy()) == bytes(out[:96].cpu().numpy())))
    del mwork
    # the route through coefficients: inverse NTT, then open over the monomial powers
    coeffs = torch.empty(32 * n, dtype=torch.uint8, device=dev)
    nwork = torch.empty(kzgpot.fr_ntt_workspace(exp, 1), dtype=torch.uint8, device=dev)
    owork = torch.empty(kzgpot.kzg_open_workspace(n), dtype=torch.uint8, device=dev)

    def by_coefficients():
        D.fr_ntt_dev(evals, exp, coeffs, inverse=True, work=nwork)
        D.g1_kzg_open_dev(bases, coeffs, z, out, key, work=owork)

    old = timed(dev, by_coefficients, reps)
    add(dict(old, what="inverse ntt + open over the monomial powers", exp=exp,
             workspace_bytes=int(nwork.numel() + owork.numel()) + 32 * n))
    ntt = timed(dev, lambda: D.fr_ntt_dev(evals, exp, coeffs, inverse=True, work=nwork), reps)
    add(dict(ntt, what="inverse ntt alone", exp=exp))
    add({"what": "summary", "exp": exp, "open_evals_min_ms": opn["min_ms"], "msm_min_ms": msm["min_ms"],
         "open_minus_msm_ms": round(opn["min_ms"] - msm["min_ms"], 4),
         "open_minus_msm_over_msm": round((opn["min_ms"] - msm["min_ms"]) / msm["min_ms"], 4),
         "fr_part_alone_min_ms": fr["min_ms"], "by_coefficients_min_ms": old["min_ms"],
         "open_evals_over_by_coefficients": round(opn["min_ms"] / old["min_ms"], 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exps", default="16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fr-only", action="store_true", help="the Fr part alone (for a kernel-trace run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "open_evals_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2029)
    res = {"tool": "tools/open_evals_timing.py", "device": torch.cuda.get_device_name(0), "version": kzgpot.version(),
           "bytes_per_evaluation": {"read": 96, "written": 64}, "inversion_share_of_the_fr_part": "not measured",
           "rows": []}

    def add(row):
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    for exp in [int(e) for e in a.exps.split(",") if e]:
        fr_rows(dev, rng, exp, a.reps, add)
        if not a.fr_only:
            open_rows(dev, rng, exp, a.reps, add)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
