"""Paired timing of the resumable chunked minn_rtl detector (MinnRTLChunkedDetector.push,
ofs_minn_rtl_chunk) against the one-shot call minn_rtl_batched makes (ofs_minn_rtl on its integer-exact
plan, rtl_exact_kernel) on the same B x Tc int16 batch, one branch, one build, one process.  Both arms
write all eight arrays and run the gate into buffers allocated once; the one-shot arm is the library
call itself so that neither arm allocates or synchronises inside the timed loop.

A push computes Tc + 3Q samples per stream (the 3Q history rows refill the lag words and the prefix
rings), stores Tc, and moves the state: 128 B header + 3Q words read and as much written per branch.
The record carries both models: (Tc + 3Q) / Tc on the compute side and 1 + state bytes / (54 B x Tc) on
the traffic side (4 B in, 6 x 8 + 2 B out per sample).  The one-shot arm runs twice per round (A/A):
the spread of its two medians is the resolution of the ratio.  A record, not a gate.

    python tools/rtl_chunk_ab.py [--B 4096 --Q 64 --Tc 1024,4096,16384 --floor-Tc 4096]
                                 [--out profiles/rtl_chunked_ab.jsonl]

The order of the arms rotates every round; each round times `--steps` back-to-back launches between
two events.  The first push on fresh streams is checked bit for bit against the one-shot arrays and
events before anything is timed.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ofdm-sync-math_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from ofdm_sync_amd import _lib, minn_rtl, synth  # noqa: E402
from bench_configs import int12  # noqa: E402
from chunk_ab_common import timed  # noqa: E402

KEYS = ("corr_total", "corr_positive", "smooth_metric", "energy_total", "corr_scaled", "energy_scaled",
        "metric_valid", "above_threshold")
SHIFT, THR, FRAC, HYST, TOFF, MAX_EV = 3, 3276, 15, 2, 0, 16


class OneShot:
    """ofs_minn_rtl on buffers allocated once (what minn_rtl_batched launches)."""

    def __init__(self, x, Q, mode):
        B, nb, T = x.shape[0], x.shape[1], x.shape[2]
        dev = x.device
        self.out = minn_rtl.MinnRTLBatch(*[torch.empty((B, T), dtype=torch.bool if k in KEYS[6:] else torch.float64,
                                                       device=dev) for k in KEYS])
        self.out.n_events = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.out.events = torch.zeros((B, MAX_EV, 4), dtype=torch.int64, device=dev)
        self.out.open_gate_start = torch.zeros((B,), dtype=torch.int64, device=dev)
        o = self.out
        self.args = (_lib.CI16, x.data_ptr(), B, nb, T, Q, SHIFT, minn_rtl._SMOOTH_MODES[mode], THR, FRAC,
                     *[getattr(o, k).data_ptr() for k in KEYS], 1, HYST, TOFF, MAX_EV, o.n_events.data_ptr(),
                     o.events.data_ptr(), o.open_gate_start.data_ptr())
        self.plan = int(_lib.lib().ofs_rtl_plan(_lib.CI16, nb, T, Q))
        self.fn = _lib.lib().ofs_minn_rtl

    def run(self):
        _lib.check(self.fn(*self.args, _lib.stream_ptr()), "ofs_minn_rtl")
        return self.out


def measure(B, Q, Tc, mode, a, dev, st):
    x = int12(synth.make_aa_batch(B, Tc, Q, seed=7, device=dev))
    if x.dim() == 3:
        x = x[:, None]
    x = x.contiguous()
    one = OneShot(x, Q, mode)
    assert 2000 <= one.plan <= 2999, one.plan
    chk = minn_rtl.MinnRTLChunkedDetector(B, Q, 1, smooth_shift=SHIFT, threshold_value=THR, threshold_frac_bits=FRAC,
                                          smooth_mode=mode, hysteresis=HYST, timing_offset=TOFF, max_events=MAX_EV)
    ref, got = one.run(), chk.push(x)
    torch.cuda.synchronize()
    for k in KEYS + ("n_events", "open_gate_start"):
        assert torch.equal(getattr(ref, k), getattr(got, k)), f"Tc={Tc}: {k} differs from the one-shot call"
    n = ref.n_events.clamp(max=MAX_EV)
    m = torch.arange(MAX_EV, device=dev)[None, :, None] < n[:, None, None]
    assert torch.equal(ref.events * m, got.events * m), f"Tc={Tc}: events differ from the one-shot call"
    arms = [("one_shot", one.run), ("chunked", lambda: chk.push(x)), ("one_shot_again", one.run)]
    ms = {name: [] for name, _ in arms}
    for _, fn in arms:
        timed(fn, a.warmup, st)
    for r in range(a.rounds):
        k = r % len(arms)
        for name, fn in arms[k:] + arms[:k]:
            ms[name].append(timed(fn, a.steps, st))
    o, c, o2 = (statistics.median(ms[k]) for k in ("one_shot", "chunked", "one_shot_again"))
    state = int(_lib.lib().ofs_rtl_chunk_state_bytes(1, Q))
    moved = 2 * 128 + state - 128                                  # header read + written, one slot read, one written
    rng = lambda v: [round(min(v), 5), round(max(v), 5)]           # noqa: E731
    row = dict(tool="rtl_chunk_ab", B=B, Q=Q, Tc=Tc, in_fmt="int16", n_br=1, smooth_mode=mode, smooth_shift=SHIFT,
               plan_one_shot=one.plan, one_shot_ms=round(o, 5), one_shot_range=rng(ms["one_shot"]),
               chunked_ms=round(c, 5), chunked_range=rng(ms["chunked"]),
               one_shot_again_ms=round(o2, 5), one_shot_again_range=rng(ms["one_shot_again"]),
               ratio=round(c / o, 4), aa_ratio=round(o2 / o, 4),
               model_compute_ratio=round((Tc + 3 * Q) / Tc, 4), model_traffic_ratio=round(1 + moved / (54 * Tc), 4),
               state_bytes_per_stream=state, state_bytes_moved_per_call=moved,
               events_mean=round(float(ref.n_events.float().mean()), 3),
               steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(dev))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--Q", type=int, default=64)
    ap.add_argument("--Tc", default="1024,4096,16384")
    ap.add_argument("--floor-Tc", type=int, default=4096, help="Tc of the floor-mode row (0: none)")
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
        rows.append(measure(a.B, a.Q, Tc, "float", a, dev, st))
        torch.cuda.empty_cache()
    if a.floor_Tc:
        rows.append(measure(a.B, a.Q, a.floor_Tc, "floor", a, dev, st))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
