"""Timing record of the group FFT (kzgpot_g1_fft_dev / kzgpot_g2_fft_dev, csrc/fft_kernels.hip) on
device-resident subgroup points from the synthetic generator, and of prepare_phase2 end to end.

    python3 tools/lagrange_timing.py [--g1 16,20] [--g2 16,18] [--e2e-log2 21] > profiles/TAG_lagrange.json

A record, not a gate: nothing comparable exists to measure against (the reference's stack does not
run here and oracle/ has no group FFT), so no speed-up over a CPU is claimed. Reported next to the
shader clock (k_clock_probe): butterflies/s (exp m/2 butterflies per transform), scalar
multiplications/s (a butterfly with twiddle 1 has none; the inverse adds one per point for 1/m) and
that rate as a fraction of a ceiling derived from the project's own measured primitive peaks:

  DESIGN.md §4 "The same roof counted in field operations" gives the chip-wide peaks of the
  Montgomery reductions at 2,338 MHz (G/s): fp_sqr 88.8, fp_mul 72.6, fp_mul_addsqr 54.1,
  fp_mul_sum2 52.0, fp_mul_sum3 34.2, f30_sqr 93.7, f30_mul 75.0; the codecs run at 0.99-1.03 of
  the time those peaks predict. Counting csrc/curve.hpp:
    G1 jac_dbl   3 S + 2 M + 1 mul+sqr                       = 0.0798 ns chip-wide
    G1 jac_madd  3 S + 6 M + 1 two-product                   = 0.1357 ns
    G2 jac_dbl   6 M + 4 two-product + 2 three-product       = 0.2180 ns
    G2 jac_madd  6 M + 16 two-product                        = 0.3903 ns
    inversion    382 S + 75 M on the radix-2^30 core          = 5.08 ns (+ ~14 M / ~40 M of tail)
  One scalar multiplication is 255 doublings and, for a random 255-bit scalar, 127.5 additions;
  a butterfly adds 2 additions and the shared inversion:
    G1  255 x 0.0798 + 129.5 x 0.1357 + 5.08 + 0.2 = 43.2 ns  -> 23.2 M/s
    G2  255 x 0.2180 + 129.5 x 0.3903 + 5.08 + 0.8 = 112.0 ns ->  8.9 M/s
  scaled by measured clock / 2,338 MHz. (The doublings alone would allow 49 M/s in G1: half of a
  butterfly's time is the ladder's additions.)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "kzg-setup-powersoftau_amd"))
import kzgpot  # noqa: E402
from kzgpot import device as D  # noqa: E402

PEAK_MHZ = 2338.0
PEAK = {"S": 88.8, "M": 72.6, "MS": 54.1, "M2": 52.0, "M3": 34.2, "S30": 93.7, "M30": 75.0}  # G reductions/s


def ns(**counts):
    return sum(k / PEAK[name] for name, k in counts.items())


def ceiling_ns(g2: bool) -> float:
    """Chip-wide ns per scalar multiplication with its butterfly tail, at PEAK_MHZ."""
    inv = ns(S30=382, M30=75)
    if g2:
        dbl, madd, tail = ns(M=6, M2=4, M3=2), ns(M=6, M2=16), ns(M2=40)
    else:
        dbl, madd, tail = ns(S=3, M=2, MS=1), ns(S=3, M=6, M2=1), ns(M=14)
    return 255 * dbl + 129.5 * madd + inv + tail


def time_fft(g2: bool, exp: int, src: torch.Tensor, launches: int):
    dev = src.device
    rec, m = (192 if g2 else 96), 1 << exp
    x = src[: m * rec]
    out = torch.empty_like(x)
    key = torch.empty(1, dtype=torch.int64, device=dev)
    work = torch.empty(kzgpot.group_fft_workspace(g2, exp), dtype=torch.uint8, device=dev)
    rows = []
    for _ in range(launches):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        c0 = D.clock_probe(dev)
        ev[0].record()
        D.group_fft_dev(g2, x, exp, out, key, inverse=True, work=work)
        ev[1].record()
        c1 = D.clock_probe(dev)
        torch.cuda.synchronize()
        clk = D.clock_mhz(c0, c1)
        rows.append((ev[0].elapsed_time(ev[1]), clk["mean"] if clk else None))
    ms, mhz = min(rows, key=lambda r: r[0])
    butterflies = exp * m // 2
    ladders = butterflies - (m - 1) + (m if exp else 0)  # twiddle-1 butterflies have none; + the 1/m pass
    ceil_at_clock = 1e3 / ceiling_ns(g2) * ((mhz or PEAK_MHZ) / PEAK_MHZ)  # M scalar multiplications/s
    return {"group": "g2" if g2 else "g1", "exp": exp, "inverse": True, "ms_per_launch": [round(r[0], 3) for r in rows],
            "best_ms": round(ms, 3), "shader_mhz": round(mhz) if mhz else None, "butterflies": butterflies,
            "scalar_multiplications": ladders, "butterflies_per_s": butterflies / ms * 1e3,
            "scalar_multiplications_per_s": ladders / ms * 1e3,
            "ceiling_M_scalar_multiplications_per_s": round(ceil_at_clock, 2),
            "fraction_of_ceiling": round(ladders / ms * 1e3 / (ceil_at_clock * 1e6), 3),
            "all_accepted": D.read_key(key) == (1 << 64) - 1}


def e2e(n_log2: int, dev):
    """prepare_phase2_buffer at exp = n_log2 on a synthetic ceremony (bench.py's helper, unchanged)."""
    sys.path.insert(0, ROOT)
    import bench

    tr, _ = bench.e2e_transcript(n_log2, 77, dev, D)
    t0 = time.perf_counter()
    out = kzgpot.prepare_phase2_buffer(tr, n_log2, n_log2)
    return {"n_log2": n_log2, "exp": n_log2, "seconds": round(time.perf_counter() - t0, 3), "bytes_out": len(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--g1", default="16,20")
    ap.add_argument("--g2", default="16,18")
    ap.add_argument("--launches", type=int, default=2)
    ap.add_argument("--e2e-log2", type=int, default=21, help="0: skip the end-to-end row")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"tool": "tools/lagrange_timing.py", "device": torch.cuda.get_device_name(0), "version": kzgpot.version(),
           "ceiling_ns_at_2338MHz": {"g1": round(ceiling_ns(False), 2), "g2": round(ceiling_ns(True), 2)}, "rows": []}
    for g2, exps in ((False, a.g1), (True, a.g2)):
        exps = [int(e) for e in exps.split(",") if e]
        if not exps:
            continue
        _, ark = D.synth("g2" if g2 else "g1", 5, 0, 1 << max(exps), dev)
        for exp in exps:
            res["rows"].append(time_fft(g2, exp, ark, a.launches))
            print(json.dumps(res["rows"][-1]), file=sys.stderr, flush=True)
        del ark
        torch.cuda.empty_cache()
    if a.e2e_log2:
        res["prepare_phase2"] = e2e(a.e2e_log2, dev)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
