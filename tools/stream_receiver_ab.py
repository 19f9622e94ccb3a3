"""Cost of the compact capture and of the receive step without a host synchronisation, against the slot
form, one build, one process (B = 4096 streams, one branch, complex64, F = H = 8192, 4096 samples per
push: the shape of profiles/frame_capture_ab.jsonl).  A record, not a gate.

    python tools/stream_receiver_ab.py [--out profiles/stream_receiver_ab.jsonl]
    rocprofv3 --kernel-trace -d OUT -o sr --output-format csv -- \\
        python tools/stream_receiver_ab.py --parts capture --kinds idle --rounds 2
    python tools/stream_receiver_ab.py --trace OUT/*/sr_kernel_trace.csv [--out ...]

Kinds: idle (no trigger), sparse (every 64th stream emits one frame per push), emit (every stream does).
A frame starts F - Tc samples before its push's chunk, so half of it comes from the ring.

capture rows: FrameCapture.push_compact against FrameCapture.push, device time between two events over
``--steps`` pushes enqueued back to back; three arms per round, order rotating: the slot form twice (two
objects: their difference is the A/A spread of this run) and the compact form.
step rows: the whole receive step.  Slot form: push + live() + receiver_backend_batched(origin=start) (no
back-end call when live() returns no frame), twice (A/A).  Device form: StreamReceiver.push.  All three
with a synchronise after every step, wall clock per step; the device form also with 16 steps enqueued
back to back and one synchronise (wall clock / 16).
--trace: median duration of the count kernel, the scan kernel and the gather / update kernels of both forms.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ofdm-sync-math_amd"))

N_FFT, CP, U = 1024, 72, 600
PILOT, DATA = 256, 256 + N_FFT + CP


def trace(path, out):
    med = lambda v: round(statistics.median(v) / 1e3, 2) if v else None  # noqa: E731
    rows = list(csv.DictReader(open(path)))
    dur = lambda m: [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if m(r["Kernel_Name"])]  # noqa: E731
    scan = dur(lambda n: "frame_scan_kernel" in n)
    r = dict(tool="stream_receiver_kt", launches=len(scan), count_us=med(dur(lambda n: "frame_count_kernel" in n)),
             scan_us=med(scan),
             scan_range_us=[round(min(scan) / 1e3, 2), round(max(scan) / 1e3, 2)] if scan else None,
             gather_compact_us=med(dur(lambda n: "frame_gather_kernel" in n and "true" in n)),
             update_compact_us=med(dur(lambda n: "frame_update_kernel" in n and "true" in n)),
             gather_slot_us=med(dur(lambda n: "frame_gather_kernel" in n and "true" not in n)),
             update_slot_us=med(dur(lambda n: "frame_update_kernel" in n and "true" not in n)))
    emit(r, out)


def emit(r, out):
    print(json.dumps(r), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as fh:
            fh.write(json.dumps(r) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--F", type=int, default=8192)
    ap.add_argument("--Tc", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kinds", default="idle,sparse,emit")
    ap.add_argument("--parts", default="capture,step")
    ap.add_argument("--trace", default=None, help="a rocprofv3 kernel trace (csv) to summarise instead of measuring")
    ap.add_argument("--out", default=None, help="append one JSON line per row to this file")
    a = ap.parse_args()
    if a.trace:
        return trace(a.trace, a.out)

    import numpy as np
    import torch
    from ofdm_sync_amd import core
    from ofdm_sync_amd.capture import FrameCapture, StreamReceiver
    from chunk_ab_common import bits, timed

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    B, F, Tc = a.B, a.F, a.Tc
    assert Tc <= F and DATA + N_FFT + CP <= F
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn((B, 1, Tc), dtype=torch.complex64, device=dev, generator=g)
    rng = np.random.default_rng(1)
    pil, dat = np.exp(2j * np.pi * rng.random(U)), np.exp(2j * np.pi * rng.random(U))
    kw = dict(n_fft=N_FFT, cp_len=CP, fs_hz=15.36e6, bins=core.centered_subcarrier_indices(U))
    span = lambda v: [round(min(v), 5), round(max(v), 5)]  # noqa: E731
    med = statistics.median
    base = dict(B=B, n_branch=1, F=F, H=F, max_pending=2, Tc=Tc, in_fmt="complex64", steps=a.steps, rounds=a.rounds,
                device=torch.cuda.get_device_name(dev))

    class Feed:
        """One capture with its own triggers: the frame that completes with each push, in every `every`-th stream."""

        def __init__(self, every, rows=None):
            self.cap = FrameCapture(B, 1, frame_len=F, dtype=torch.complex64, device=dev, compact_rows=rows)
            self.count = ((torch.arange(B, device=dev) % every == 0).to(torch.int32) if every
                          else torch.zeros(B, dtype=torch.int32, device=dev))
            n_warm = F // Tc                                       # pushes before the first frame can complete
            for _ in range(n_warm):
                self.cap.push(x)
            self.trig = torch.full((B, 1), (n_warm + 1) * Tc - F, dtype=torch.int64, device=dev)

        def push(self):
            r = self.cap.push(x, self.trig, self.count)
            self.trig.add_(Tc)
            return r

        def push_compact(self):
            r = self.cap.push_compact(x, self.trig, self.count)
            self.trig.add_(Tc)
            return r

    def rotate(arms, fn_time):
        ms = {n: [] for n, _ in arms}
        for _, fn in arms:
            fn_time(fn, a.warmup)
        for r in range(a.rounds):
            for name, fn in arms[r % len(arms):] + arms[:r % len(arms)]:
                ms[name].append(fn_time(fn, a.steps))
        return ms

    def wall_sync(fn, steps):                                     # a synchronise after every step
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
            torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def wall_ahead(fn, steps):                                    # `steps` steps enqueued, one synchronise
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for kind, every in (("idle", 0), ("sparse", 64), ("emit", 1)):
        if kind not in a.kinds.split(","):
            continue
        n_emit = 0 if not every else (B + every - 1) // every
        rows = max(n_emit, 64)
        if "capture" in a.parts.split(","):
            fa, fb, fc = Feed(every), Feed(every), Feed(every, rows)
            ra, rc = fa.push(), fc.push_compact()                 # one push checked before anything is timed
            sb, _, frames, start = fa.cap.live(ra)
            assert rc.n_rows.tolist() == [n_emit, 0] and torch.equal(rc.frame_start[:n_emit], start)
            assert torch.equal(bits(rc.frames[:n_emit]), bits(frames)), "compact frames differ from the slot form's"
            fb.push()
            ms = rotate([("slot_a", fa.push), ("compact", fc.push_compact), ("slot_b", fb.push)],
                        lambda fn, n: timed(fn, n, st))
            sa, sb_, c = med(ms["slot_a"]), med(ms["slot_b"]), med(ms["compact"])
            s = 0.5 * (sa + sb_)
            emit(dict(tool="stream_receiver_ab", part="capture", kind=kind, frames_per_push=n_emit, compact_rows=rows,
                      slot_ms=round(s, 5), slot_a_ms=round(sa, 5), slot_b_ms=round(sb_, 5), slot_a_range=span(ms["slot_a"]),
                      slot_b_range=span(ms["slot_b"]), aa_spread=round(abs(sa - sb_) / s, 5), compact_ms=round(c, 5),
                      compact_range=span(ms["compact"]), ratio=round(c / s, 4), excess_us=round((c - s) * 1e3, 2), **base),
                 a.out)
            del fa, fb, fc
            torch.cuda.empty_cache()
        if "step" in a.parts.split(","):
            fa, fb, fc = Feed(every), Feed(every), Feed(every, rows)
            rx = StreamReceiver(fc.cap, PILOT, DATA, pil, dat, **kw)

            def slot_step(f):
                def step():
                    _, _, frames, start = f.cap.live(f.push())
                    if len(start):
                        return core.receiver_backend_batched(frames, PILOT, DATA, pil, dat, origin=start, **kw)
                return step

            def device_step():
                r = rx.push(x, fc.trig, fc.count)
                fc.trig.add_(Tc)
                return r

            ref = slot_step(fa)()
            res, dec = device_step()
            torch.cuda.synchronize()
            if n_emit:
                assert torch.equal(bits(dec["xa"][:n_emit]), bits(ref["xa"])), "decoded words differ from the slot form's"
            slot_step(fb)()
            ms = rotate([("slot_a", slot_step(fa)), ("device", device_step), ("slot_b", slot_step(fb))], wall_sync)
            ahead = [wall_ahead(device_step, 16) for _ in range(a.rounds + 1)][1:]
            sa, sb_, d, h = med(ms["slot_a"]), med(ms["slot_b"]), med(ms["device"]), med(ahead)
            s = 0.5 * (sa + sb_)
            emit(dict(tool="stream_receiver_ab", part="step", kind=kind, frames_per_push=n_emit, compact_rows=rows,
                      n_fft=N_FFT, cp_len=CP, n_used=U, slot_sync_ms=round(s, 5), slot_a_ms=round(sa, 5),
                      slot_b_ms=round(sb_, 5), slot_a_range=span(ms["slot_a"]), slot_b_range=span(ms["slot_b"]),
                      aa_spread=round(abs(sa - sb_) / s, 5), device_sync_ms=round(d, 5), device_sync_range=span(ms["device"]),
                      device_ahead16_ms=round(h, 5), device_ahead16_range=span(ahead), ratio_sync=round(d / s, 4),
                      ratio_ahead16=round(h / s, 4), **base), a.out)
            del fa, fb, fc, rx
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
