"""Paired timing of the resumable chunked zc_v2 CFAR + gate (ZCChunkedDetector.push_mag,
ofs_zc_detect_chunk) against the unchanged one-shot call (ofs_zc_detect) on the same B x Tc float64
magnitude batch, one build, one process.  Both arms write into buffers allocated once; neither allocates
or synchronises inside the timed loop.  Default mode: events + gate_mask only (the benchmarked mode of the
one-shot call); --state-Tc adds one row with the five state arrays.

A push walks Tc samples per stream like the one-shot call, but its c[n - W] comes from the carried history
for the first W samples and it writes the last min(W, Tc) magnitudes back.  The record carries two models,
neither a promise: (Tc + W) / Tc on the compute side (a one-shot call over history and chunk) and
1 + 16 W / (9 Tc) on the traffic side (history read and written against 8 B in + 1 B out per sample).
The one-shot kernel is bound by its dependent fp64 chain, not by traffic.  The one-shot arm runs twice per
round (A/A): the spread of its two medians is the resolution of the ratio.  A fourth arm runs the one-shot
call on its register-staged tiles (variant ZC_NODMA), the kernel form the push is built from.  A record,
not a gate.

    python tools/zc_chunk_ab.py [--B 4096 --W 2048 --hyst 256 --Tc 1024,4096,16384 --state-Tc 4096]
                                [--out profiles/zc_chunked_ab.jsonl]

The order of the arms rotates every round; each round times `--steps` back-to-back launches between two
events.  A final push on fresh streams is checked bit for bit against the one-shot outputs before anything
is timed; the timed pushes continue one stream (the window is full: the steady state of a receiver).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ofdm-sync-math_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_sync_amd import _lib, zc_v2  # noqa: E402
from chunk_ab_common import timed  # noqa: E402

STATE = ("local_sum", "corr_scaled", "thresh_scaled", "above_threshold", "metric_valid")
FRAC, MIN_MAG, REFLEN, MAX_EV = 15, 0.3, 2048, 64


def make_mag(B, Tc, dev):
    """|N(0, 1)| with a pulse of 8-20 every ~1500 samples in every other stream."""
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    c = torch.randn((B, Tc), dtype=torch.float64, device=dev, generator=g).abs_()
    rng = np.random.default_rng(7)
    for p in range(700, Tc - 4, 1500):
        c[::2, p + int(rng.integers(0, 64))] = float(rng.uniform(8.0, 20.0))
    return c


class OneShot:
    """ofs_zc_detect on buffers allocated once."""

    def __init__(self, mag, W, tv, hyst, state):
        B, n = mag.shape
        dev = mag.device
        self.arr = {k: torch.empty((B, n), dtype=torch.float64 if k in STATE[:3] else torch.uint8, device=dev)
                    for k in (STATE if state else ())}
        self.gate_mask = torch.empty((B, n), dtype=torch.uint8, device=dev)
        self.n_events = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.events = torch.zeros((B, MAX_EV, 4), dtype=torch.int64, device=dev)
        self.peak_values = torch.zeros((B, MAX_EV), dtype=torch.float64, device=dev)
        self.args = (mag.data_ptr(), B, n, W, tv, FRAC, MIN_MAG, REFLEN, hyst,
                     *[_lib.ptr(self.arr.get(k)) for k in STATE], self.gate_mask.data_ptr(), MAX_EV,
                     self.n_events.data_ptr(), self.events.data_ptr(), self.peak_values.data_ptr())
        self.plan = int(_lib.lib().ofs_zc_detect_plan(n, W, hyst, int(state), int(mag.data_ptr() % 16 == 0)))
        self.fn = _lib.lib().ofs_zc_detect

    def run(self):
        _lib.check(self.fn(*self.args, _lib.stream_ptr()), "ofs_zc_detect")
        return self


def measure(B, W, hyst, Tc, state, a, dev, st):
    tv = int(4.0 * (1 << FRAC) / W)
    mag = make_mag(B, Tc, dev)
    one = OneShot(mag, W, tv, hyst, state)
    chk = zc_v2.ZCChunkedDetector(B, np.ones(REFLEN, complex), 1, window_size=W, thresh_value=tv, thresh_frac_bits=FRAC,
                                  min_corr_mag=MIN_MAG, hysteresis=hyst, max_events=MAX_EV,
                                  outputs=(STATE if state else ()) + ("gate_mask",))
    ref, got = one.run(), chk.push_mag(mag, final=True)
    torch.cuda.synchronize()
    for k in one.arr:
        assert torch.equal(one.arr[k], getattr(got, k)), f"Tc={Tc}: {k} differs from the one-shot call"
    assert torch.equal(ref.gate_mask, got.gate_mask), f"Tc={Tc}: gate_mask differs from the one-shot call"
    assert int(ref.n_events.max()) <= MAX_EV, f"Tc={Tc}: {int(ref.n_events.max())} events in one stream, {MAX_EV} slots"
    assert torch.equal(ref.n_events, got.n_events), f"Tc={Tc}: n_events differ from the one-shot call"
    m = torch.arange(MAX_EV, device=dev)[None, :] < ref.n_events[:, None]
    assert torch.equal(ref.events * m[:, :, None], got.events * m[:, :, None]), f"Tc={Tc}: events differ"
    assert torch.equal(ref.peak_values * m, got.peak_values * m), f"Tc={Tc}: peak values differ"
    assert not chk.state.any().item()
    # fourth arm: the one-shot call forced onto its register-staged tiles (variant ZC_NODMA, plan 1), the
    # kernel form the push is built from - it separates "no LDS-DMA" from what carrying the state costs
    reg = {"ZC_NODMA": 1}
    with _lib.variants(**reg):
        plan_reg = int(_lib.lib().ofs_zc_detect_plan(Tc, W, hyst, int(state), int(mag.data_ptr() % 16 == 0)))
    arms = [("one_shot", one.run, {}), ("chunked", lambda: chk.push_mag(mag), {}), ("one_shot_again", one.run, {}),
            ("one_shot_register_tiles", one.run, reg)]
    ms = {name: [] for name, _, _ in arms}

    def arm(fn, var, steps):
        with _lib.variants(**var):
            return timed(fn, steps, st)

    for _, fn, var in arms:
        arm(fn, var, a.warmup)
    for r in range(a.rounds):
        k = r % len(arms)
        for name, fn, var in arms[k:] + arms[:k]:
            ms[name].append(arm(fn, var, a.steps))
    o, c, o2, o_reg = (statistics.median(ms[k]) for k in ("one_shot", "chunked", "one_shot_again",
                                                          "one_shot_register_tiles"))
    sbytes = int(_lib.lib().ofs_zc_chunk_state_bytes(W))
    rng = lambda v: [round(min(v), 5), round(max(v), 5)]           # noqa: E731
    row = dict(tool="zc_chunk_ab", B=B, W=W, hysteresis=hyst, Tc=Tc, mode="state arrays" if state else "events + mask",
               plan_one_shot=one.plan, one_shot_ms=round(o, 5), one_shot_range=rng(ms["one_shot"]),
               chunked_ms=round(c, 5), chunked_range=rng(ms["chunked"]),
               one_shot_again_ms=round(o2, 5), one_shot_again_range=rng(ms["one_shot_again"]),
               one_shot_register_tiles_ms=round(o_reg, 5), plan_register_tiles=plan_reg,
               ratio=round(c / o, 4), aa_ratio=round(o2 / o, 4), ratio_to_register_tiles=round(c / o_reg, 4),
               model_compute_ratio=round((Tc + W) / Tc, 4), model_traffic_ratio=round(1 + 16 * W / (9 * Tc), 4),
               state_bytes_per_stream=sbytes, events_mean=round(float(ref.n_events.float().mean()), 3),
               steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(dev))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--W", type=int, default=2048)
    ap.add_argument("--hyst", type=int, default=256)
    ap.add_argument("--Tc", default="1024,4096,16384")
    ap.add_argument("--state-Tc", type=int, default=4096, help="Tc of the row with state arrays (0: none)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="append one JSON line per row to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    rows = []
    for Tc in [int(v) for v in a.Tc.split(",")]:
        rows.append(measure(a.B, a.W, a.hyst, Tc, False, a, dev, st))
        torch.cuda.empty_cache()
    if a.state_Tc:
        rows.append(measure(a.B, a.W, a.hyst, a.state_Tc, True, a, dev, st))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
