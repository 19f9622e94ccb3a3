"""Diagnostic: where a push of the chunked zc_v2 CFAR + gate spends its time, per role and phase
(zc_chunk_kernel built with -DOFS_ZC_CHUNK_TIMING=1), next to the one-shot kernel on its register-staged
tiles (zc_cfar_kernel built with -DOFS_ZC_TIMING=1, variant ZC_NODMA) on the same batch.

    python tools/variants.py zc_chunk.hip "zcchunktime=-DOFS_ZC_CHUNK_TIMING=1"
    python tools/variants.py zc_cfar.hip "zctime=-DOFS_ZC_TIMING=1"
    OFS_LIB=build/libofdmsync_zcchunktime.so python tools/zc_chunk_phase.py [--out FILE.jsonl]
    OFS_LIB=build/libofdmsync_zctime.so python tools/zc_chunk_phase.py --one-shot [--out FILE.jsonl]

One process per build, no tracing.  The counter is s_memtime, read by lane 0 of every wave (on gfx950 it
runs at about the shader clock: a wave's life of 0.25 ms is ~5e5 ticks); ticks are summed over the waves of
a role and divided by the number of such waves and launches, so every figure is "thousands of ticks of one
wave's life per launch", with each phase's share of that life next to it.  4096 streams are 512 workgroups
of 58 KB LDS, two per CU on 256 CUs: one round, so a wave's life is the launch without its ramp.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ofdm-sync-math_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_sync_amd import _lib, zc_v2  # noqa: E402
if os.environ.get("OFS_LIB"):   # a tools/variants.py tuning build, named explicitly (not a product switch)
    _lib.use_tuning_library(os.environ["OFS_LIB"])
from zc_chunk_ab import FRAC, MAX_EV, MIN_MAG, REFLEN, OneShot, make_mag, timed  # noqa: E402

PHASES = ("entry", "tile loads + staging", "chain / helper work", "chunk barrier", "full barrier after the loop",
          "ring write-back + second full barrier", "headers and counts")
CFAR_ROLES = ("walker: tile wait (LDS-DMA form only)", "walker: tile loads + staging + chain", "walker: barrier",
              "helpers: work", "helpers: barrier")


def table(names, v):
    """{phase: [thousands of ticks, share of the wave's life]}"""
    tot = sum(v) or 1.0
    return {k: [round(x, 1), round(x / tot, 3)] for k, x in zip(names, v)}


def chunked(B, W, hyst, Tc, state, steps, dev, st):
    tv = int(4.0 * (1 << FRAC) / W)
    mag = make_mag(B, Tc, dev)
    names = ("local_sum", "corr_scaled", "thresh_scaled", "above_threshold", "metric_valid") if state else ()
    chk = zc_v2.ZCChunkedDetector(B, np.ones(REFLEN, complex), 1, window_size=W, thresh_value=tv, thresh_frac_bits=FRAC,
                                  min_corr_mag=MIN_MAG, hysteresis=hyst, max_events=MAX_EV, outputs=names + ("gate_mask",))
    f = _lib.lib().ofs_zc_chunk_prof
    f.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
    buf = (ctypes.c_ulonglong * 16)()
    timed(lambda: chk.push_mag(mag), 3, st)                    # fills the window, warms up
    assert f(buf) == 0
    ms = timed(lambda: chk.push_mag(mag), steps, st)
    assert f(buf) == 0
    nwg = (B + 7) // 8
    walker = [buf[i] / 1e3 / (steps * nwg) for i in range(7)]
    helper = [buf[8 + i] / 1e3 / (steps * nwg * 3) for i in range(7)]
    return dict(tool="zc_chunk_phase", kernel="zc_chunk_kernel", B=B, W=W, hysteresis=hyst, Tc=Tc,
                mode="state arrays" if state else "events + mask", ms_per_launch_timing_build=round(ms, 5),
                walker_kticks=table(PHASES, walker), walker_life_kticks=round(sum(walker), 1),
                helper_kticks=table(PHASES, helper), helper_life_kticks=round(sum(helper), 1), steps=steps)


def one_shot(B, W, hyst, Tc, state, steps, dev, st):
    tv = int(4.0 * (1 << FRAC) / W)
    mag = make_mag(B, Tc, dev)
    one = OneShot(mag, W, tv, hyst, state)
    f = _lib.lib().ofs_zc_prof
    f.argtypes = [ctypes.POINTER(ctypes.c_ulonglong)]
    buf = (ctypes.c_ulonglong * 5)()
    with _lib.variants(ZC_NODMA=1):
        plan = int(_lib.lib().ofs_zc_detect_plan(Tc, W, hyst, int(state), 1))
        timed(one.run, 3, st)
        assert f(buf) == 0
        ms = timed(one.run, steps, st)
        assert f(buf) == 0
    nwg = (B + 7) // 8                                          # register-staged form: 8 streams, 1 + 3 waves
    kt = [buf[i] / 1e3 / (steps * nwg * (1 if i < 3 else 3)) for i in range(5)]
    return dict(tool="zc_chunk_phase", kernel="zc_cfar_kernel, register-staged tiles", plan=plan, B=B, W=W,
                hysteresis=hyst, Tc=Tc, mode="state arrays" if state else "events + mask",
                ms_per_launch_timing_build=round(ms, 5), walker_kticks=table(CFAR_ROLES[:3], kt[:3]),
                walker_life_kticks=round(sum(kt[:3]), 1), helper_kticks=table(CFAR_ROLES[3:], kt[3:]),
                helper_life_kticks=round(sum(kt[3:]), 1), steps=steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--W", type=int, default=2048)
    ap.add_argument("--hyst", type=int, default=256)
    ap.add_argument("--Tc", default="4096,16384")
    ap.add_argument("--state-Tc", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--one-shot", action="store_true", help="time zc_cfar_kernel (OFS_ZC_TIMING build) instead")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    run = one_shot if a.one_shot else chunked
    cases = [(int(v), False) for v in a.Tc.split(",")] + ([(a.state_Tc, True)] if a.state_Tc else [])
    rows = []
    for Tc, state in cases:
        rows.append(run(a.B, a.W, a.hyst, Tc, state, a.steps, dev, st))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
