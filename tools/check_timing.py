"""Timing record of KZG10 batch_check and the pairing product (csrc/verify.hip, csrc/pairing_kernels.hip)
on device-resident data.

    python3 tools/check_timing.py [--log2 16,20] [--pairs 2,256] [--reps 5] [--out profiles/check_timing.json]
    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/check_timing.py --pairing-only --out X
    python3 tools/check_timing.py --split DIR/.../run_kernel_trace.csv --into profiles/check_timing.json

A record, not a gate: nobody has measured any of this before, no threshold is fixed in advance and no
speed-up over a CPU is claimed; a difference is formed only between rows of the same run. Device events,
one warm-up launch, `reps` timed launches reported as min / median / max, next to the shader clock
(k_clock_probe). In one process:

  1 kzgpot_kzg_batch_check_dev over n proofs (synthetic G1 points as commitments and proofs, random
    scalars: the verdict is "rejected", the work is the same) against the two MSMs alone over the same
    bases and scalar counts, 2 n + 2 and n: the difference is the Fr pass, the staging copies and the
    product of two pairings;
  2 kzgpot_pairing_product_dev alone at each pair count (generator records repeated).

The split of the pairing product into Miller loops / product tree / final exponentiation comes from a
kernel trace in a run of its own (tracing slows the host): --split sums the three kernels' durations
per pair count and adds them to the record."""
from __future__ import annotations

import argparse
import collections
import csv
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "kzg-setup-powersoftau_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def split(trace, into):
    """per (kernel, grid): calls and the mean duration; the pair count shows in k_pair_miller's grid"""
    per = collections.defaultdict(list)
    with open(trace) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            for k in ("k_pair_miller", "k_pair_tree", "k_pair_final"):
                if k in name:
                    per[(k, int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0))].append(
                        int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    rows = [{"kernel": k, "grid_threads": g, "calls": len(d), "mean_ms": round(sum(d) / len(d) / 1e6, 4),
             "min_ms": round(min(d) / 1e6, 4)} for (k, g), d in sorted(per.items())]
    with open(into) as f:
        res = json.load(f)
    res["pairing_kernel_split"] = {"source": "rocprofv3 --kernel-trace of tools/check_timing.py --pairing-only, a run of its own",
                                   "rows": rows}
    with open(into, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(rows, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", default="16,20")
    ap.add_argument("--pairs", default="2,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairing-only", action="store_true", help="the pairing product alone (for a kernel-trace run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_timing.json"))
    ap.add_argument("--split", help="a rocprofv3 kernel-trace CSV of a --pairing-only run")
    ap.add_argument("--into", default=os.path.join(ROOT, "profiles", "check_timing.json"))
    a = ap.parse_args()
    if a.split:
        return split(a.split, a.into)

    import numpy as np
    import torch

    import kzgpot
    import kzgpot_oracle as O
    from kzgpot import device as D
    from open_timing import random_bytes

    def timed(fn, reps):
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

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2030)
    res = {"tool": "tools/check_timing.py", "device": torch.cuda.get_device_name(0), "version": kzgpot.version(),
           "note": "timing record, not a gate; no CPU speed-up is claimed", "rows": []}

    def add(row):
        res["rows"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)

    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)  # noqa: E731
    g1 = O.ark_g1_serialize((O.G1_GEN[0], O.G1_GEN[1], False))
    g2 = O.ark_g2_serialize((O.G2_GEN[0], O.G2_GEN[1], False))
    key = torch.empty(1, dtype=torch.int64, device=dev)
    out = torch.empty(D.GT_OUT_BYTES, dtype=torch.uint8, device=dev)

    for k in [int(x) for x in a.pairs.split(",") if x]:
        d1, d2 = to_dev(g1 * k), to_dev(g2 * k)
        work = torch.empty(kzgpot.pairing_workspace(k), dtype=torch.uint8, device=dev)
        row = timed(lambda: D.pairing_product_dev(d1, d2, out, key, work=work), a.reps)
        add(dict(row, what="pairing product", pairs=k, workspace_bytes=int(work.numel()),
                 all_accepted=D.read_key(key) == (1 << 64) - 1, is_one=int(out[576].item())))
    if not a.pairing_only:
        vk = to_dev(g1 * 2 + g2 * 2)
        point = torch.empty(96, dtype=torch.uint8, device=dev)
        for log2 in [int(x) for x in a.log2.split(",") if x]:
            n = 1 << log2
            _, comms = D.synth("g1", 11, 0, n, dev)
            _, wits = D.synth("g1", 12, 0, n, dev)
            z, v, rv, rho = (random_bytes(rng, n, dev) for _ in range(4))
            work = torch.empty(kzgpot.kzg_batch_check_workspace(n), dtype=torch.uint8, device=dev)
            chk = timed(lambda: D.kzg_batch_check_dev(vk, comms, z, v, wits, rho, out, key, d_random_vs=rv, work=work), a.reps)
            add(dict(chk, what="kzg batch check", log2=log2, workspace_bytes=int(work.numel()),
                     all_accepted=D.read_key(key) == (1 << 64) - 1, verdict=int(out[576].item())))
            del work
            # the two MSMs alone: 2 n + 2 bases (commitments, proofs, g, gamma_g) and the n proofs
            bases = torch.cat([comms, wits, vk[:192]])
            scalars = torch.cat([rho, z, v[:64]])
            mwork = torch.empty(kzgpot.msm_workspace(False, 2 * n + 2), dtype=torch.uint8, device=dev)

            def two_msms():
                D.g1_msm_dev(wits, rho, point, key, work=mwork)
                D.g1_msm_dev(bases, scalars, point, key, work=mwork)

            msm = timed(two_msms, a.reps)
            add(dict(msm, what="the two msms alone", log2=log2, window_bits=[kzgpot.msm_window_bits(n),
                                                                             kzgpot.msm_window_bits(2 * n + 2)]))
            add({"what": "summary", "log2": log2, "batch_check_min_ms": chk["min_ms"], "two_msms_min_ms": msm["min_ms"],
                 "check_minus_msms_ms": round(chk["min_ms"] - msm["min_ms"], 4)})
            del bases, scalars, mwork, comms, wits
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
