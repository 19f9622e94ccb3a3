"""Interleaved in-process A/B of debug variants on the headline detector (cfg3: 65536 x 1024 c64,
L = 512, P/R/M + events) through the product's AABatchDetector, same buffers for every arm.
Diagnostic tooling (not the product).

    python tools/headline_ab.py --ab "FAST_SCAN=64;FAST_SCAN=32" [--reps 7] [--steps 20] [--realloc 3]

An empty variant set (";;" or a leading ";") is the default dispatch; listing it twice gives the
A/A control.  The arm order rotates by one every repetition.  --realloc N repeats the whole
comparison on N fresh detectors (the earlier ones stay allocated, so every round gets other
buffers) and prints one JSON line per allocation plus a summary: per arm the paired difference
to arm 0 (same allocation, same repetition), in percent of arm 0.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ofdm-sync-math_amd"))
from ofdm_sync_amd import _lib, synth, sync_aa  # noqa: E402


def median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])


def arm_name(vs):
    return ",".join(f"{k}={v}" for k, v in vs.items()) or "default"


def time_arms(det, sets, reps, steps):
    """times[i][r]: ms per step of arm i in repetition r (arms interleaved, order rotated per repetition)."""
    keys = sorted({k for st in sets for k in st})
    st = torch.cuda.current_stream()
    times = [[] for _ in sets]
    for r in range(reps):
        for o in range(len(sets)):
            i = (o + r) % len(sets)
            for k in keys:
                _lib.set_variant(k, None)
            for k, v in sets[i].items():
                _lib.set_variant(k, int(v))
            for _ in range(3):
                det.run()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(steps):
                det.run()
            e1.record(st)
            torch.cuda.synchronize()
            times[i].append(round(e0.elapsed_time(e1) / steps, 5))
    _lib.reset_variants()
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", required=True, help="K=V[,K2=V2][;K=V...] variant sets (ofs_debug_set_variant names)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--realloc", type=int, default=1, help="fresh detectors (allocations) to repeat the comparison on")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    sets = [dict(kv.split("=") for kv in cfg.split(",") if kv) for cfg in a.ab.split(";")]
    names = []
    for vs in sets:                                          # a repeated set (A/A) gets a suffix
        n = arm_name(vs)
        names.append(n if n not in names else f"{n}#{sum(x.split('#')[0] == n for x in names) + 1}")
    x = synth.headline_batch(a.B, 1024, 512, seed=2026, device=dev)
    held, pct = [], [[] for _ in sets]
    for alloc in range(a.realloc):
        det = sync_aa.AABatchDetector(a.B, 1024, 1, 512, outputs=("P", "R", "M"), max_events=4, device=dev)
        det.x.copy_(x)
        held.append(det)
        times = time_arms(det, sets, a.reps, a.steps)
        out = {"alloc": alloc, "placement": det.placement, "plan": det.plan(), "x_ptr": det.x.data_ptr()}
        for i, n in enumerate(names):
            d = [100.0 * (t - t0) / t0 for t, t0 in zip(times[i], times[0])]
            pct[i].append(median(d))
            out[n] = {"median_ms": median(times[i]), "paired_pct_vs_arm0": round(median(d), 3), "ms": times[i]}
        print(json.dumps(out), flush=True)
    if a.realloc > 1:
        print(json.dumps({"summary": {n: {"per_alloc_paired_pct_vs_arm0": [round(p, 3) for p in pct[i]],
                                          "median_pct": round(median(pct[i]), 3)}
                                      for i, n in enumerate(names)}}), flush=True)


if __name__ == "__main__":
    main()
