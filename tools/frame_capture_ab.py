"""Cost of the frame capture (capture.FrameCapture.push, ofs_frame_capture_chunk) against plain device
copies of the bytes it has to move, one build, one process (B = 4096 streams, one branch, complex64,
F = 8192, H = F, max_pending = 2).  A record, not a gate.

    python tools/frame_capture_ab.py [--B 4096 --F 8192 --Tc 1024,4096,16384] [--out profiles/frame_capture_ab.jsonl]

Idle rows (one per Tc): a push without any trigger - the gather's workgroups leave after reading the
header, the update kernel writes the chunk's newest min(Tc, H) samples into the ring - against a copy of
the same chunk into a preallocated buffer (what ``clone`` does after its allocation), which moves the
bytes of the ring write when Tc <= H and more when Tc > H.
Emit row (Tc = F): every stream emits one frame per push, half of it from the ring and half from the
chunk (the trigger is the chunk's first sample minus F / 2, advanced on the device after every push),
against a copy of the chunk plus a copy of B frames.  Sparse row: the same with every 64th stream
emitting, against a copy of the chunk plus B / 64 frames.
Three arms per round, order rotating: the copy twice (arms a and b: their difference is the A/A spread
of this run) and the push.  Each round times ``--steps`` repetitions between two events.  The emitted
frames of one push are checked bit for bit against the stream before anything is timed.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ofdm-sync-math_amd"))

import torch  # noqa: E402

from ofdm_sync_amd import _lib  # noqa: E402
from ofdm_sync_amd.capture import FrameCapture  # noqa: E402
from chunk_ab_common import bits, timed  # noqa: E402


def rotate(arms, rounds, steps, warmup, st):
    ms = {n: [] for n, _ in arms}
    for _, fn in arms:
        timed(fn, warmup, st)
    for r in range(rounds):
        for name, fn in arms[r % len(arms):] + arms[:r % len(arms)]:
            ms[name].append(timed(fn, steps, st))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--F", type=int, default=8192)
    ap.add_argument("--Tc", default="1024,4096,16384")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kinds", default="idle,emit,sparse", help="rows to measure: idle (one per Tc), emit, sparse")
    ap.add_argument("--out", default=None, help="append one JSON line per row to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    B, F = a.B, a.F
    g = torch.Generator(device=dev).manual_seed(3)
    rng = lambda v: [round(min(v), 5), round(max(v), 5)]  # noqa: E731
    rows = []

    def row(kind, Tc, ms, copy_bytes, push_bytes):
        ca, cb, p = (statistics.median(ms[n]) for n in ("copy_a", "copy_b", "push"))
        c = 0.5 * (ca + cb)
        r = dict(tool="frame_capture_ab", kind=kind, B=B, n_branch=1, F=F, H=F, max_pending=2, Tc=Tc,
                 in_fmt="complex64", copy_ms=round(c, 5), copy_a_ms=round(ca, 5), copy_b_ms=round(cb, 5),
                 copy_a_range=rng(ms["copy_a"]), copy_b_range=rng(ms["copy_b"]), aa_spread=round(abs(ca - cb) / c, 5),
                 push_ms=round(p, 5), push_range=rng(ms["push"]), ratio=round(p / c, 4),
                 copy_bytes=copy_bytes, push_bytes_written=push_bytes,
                 copy_GBps=round(2 * copy_bytes / c / 1e6, 1), push_GBps_written=round(push_bytes / p / 1e6, 1),
                 state_bytes_per_stream=int(_lib.lib().ofs_frame_capture_state_bytes(_lib.C64, 1, F, F, 2)),
                 steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(dev))
        rows.append(r)
        print(json.dumps(r), flush=True)

    for Tc in [int(v) for v in a.Tc.split(",")] if "idle" in a.kinds.split(",") else []:
        x = torch.randn((B, 1, Tc), dtype=torch.complex64, device=dev, generator=g)
        dst = torch.empty_like(x)
        cap = FrameCapture(B, 1, frame_len=F, dtype=torch.complex64, device=dev)
        ms = rotate([("copy_a", lambda: dst.copy_(x)), ("push", lambda: cap.push(x)), ("copy_b", lambda: dst.copy_(x))],
                    a.rounds, a.steps, a.warmup, st)
        assert int(cap.push(x).n_frames.sum().item()) == 0
        row("idle", Tc, ms, B * Tc * 8, B * min(Tc, F) * 8)
        del x, dst, cap
        torch.cuda.empty_cache()

    # emit: every stream emits one frame per push; sparse: every 64th stream does.  Tc = F, the frame
    # starts F / 2 before the chunk
    for kind, every in (("emit", 1), ("sparse", 64)):
        if kind not in a.kinds.split(","):
            continue
        Tc = F
        n_emit = (B + every - 1) // every
        x = torch.randn((B, 1, Tc), dtype=torch.complex64, device=dev, generator=g)
        dst = torch.empty_like(x)
        fsrc = torch.randn((n_emit, 1, F), dtype=torch.complex64, device=dev, generator=g)
        fdst = torch.empty_like(fsrc)
        cap = FrameCapture(B, 1, frame_len=F, dtype=torch.complex64, device=dev)
        cap.push(x)
        trig = torch.full((B, 1), Tc - F // 2, dtype=torch.int64, device=dev)
        count = (torch.arange(B, device=dev) % every == 0).to(torch.int32)

        def emit():
            r = cap.push(x, trig, count)
            trig.add_(Tc)
            return r

        def copies():
            dst.copy_(x)
            fdst.copy_(fsrc)

        r = emit()
        want = torch.cat([x[:, :, Tc - F // 2:], x[:, :, :F - F // 2]], dim=2)      # the stream is x repeated
        assert torch.equal(r.n_frames, count) and int(r.dropped.sum().item()) == 0
        assert torch.equal(bits(r.frames[::every, 0]), bits(want[::every])), "emitted frames differ from the stream"
        ms = rotate([("copy_a", copies), ("push", emit), ("copy_b", copies)], a.rounds, a.steps, a.warmup, st)
        assert int(cap.push(x, trig, count).n_frames.sum().item()) == n_emit
        row(kind, Tc, ms, (B * Tc + n_emit * F) * 8, (B * min(Tc, F) + n_emit * F) * 8)
        del x, dst, fsrc, fdst, cap
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for r in rows:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
