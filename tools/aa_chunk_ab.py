"""Paired timing of the resumable chunked [A][A] detector (AAChunkedDetector.push, ofs_aa_detect_chunk)
against the one-shot AABatchDetector on the same B x Tc int16 batch, fp64, one build, one process
(the cfg2a family: B = 4096, L = 128).  A push reads and computes Tc + 2L samples per stream, stores
Tc and moves the state (128 B header + 2L words read, 2L words written per antenna), so the model
is a ratio near (Tc + 2L) / Tc on the input / compute side with equal stores.  A record, not a gate.

    python tools/aa_chunk_ab.py [--B 4096 --L 128 --Tc 1024,4096,16384] [--out profiles/aa_chunked_ab.jsonl]

The order of the two arms rotates every round; each round times `--steps` back-to-back launches
between two events.  The first push on fresh streams is checked bit for bit against the one-shot
P / R / M before anything is timed.
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

from ofdm_sync_amd import _lib, sync_aa, synth  # noqa: E402
from bench_configs import int12  # noqa: E402
from chunk_ab_common import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--L", type=int, default=128)
    ap.add_argument("--Tc", default="1024,4096,16384")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append one JSON line per Tc to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    B, L = a.B, a.L
    rows = []
    for Tc in [int(v) for v in a.Tc.split(",")]:
        x = int12(synth.make_aa_batch(B, Tc, L, seed=7, device=dev))
        one = sync_aa.AABatchDetector(B, Tc, 1, L, precision="fp64", in_dtype=torch.int16, placement="plain")
        chk = sync_aa.AAChunkedDetector(B, 1, L, in_dtype=torch.int16)
        ref, got = one.run(x), chk.push(x)
        torch.cuda.synchronize()
        for k in ("P", "R", "M"):
            assert torch.equal(getattr(ref, k), getattr(got, k)), f"Tc={Tc}: {k} differs from the one-shot call"
        arms = [("one_shot", lambda: one.run(x)), ("chunked", lambda: chk.push(x))]
        ms = {n: [] for n, _ in arms}
        for _, fn in arms:
            timed(fn, a.warmup, st)
        for r in range(a.rounds):
            for name, fn in arms[r % 2:] + arms[:r % 2]:
                ms[name].append(timed(fn, a.steps, st))
        o, c = statistics.median(ms["one_shot"]), statistics.median(ms["chunked"])
        row = dict(tool="aa_chunk_ab", B=B, L=L, Tc=Tc, in_fmt="int16", precision="fp64", plan_one_shot=one.plan(),
                   one_shot_ms=round(o, 5), one_shot_range=[round(min(ms["one_shot"]), 5), round(max(ms["one_shot"]), 5)],
                   chunked_ms=round(c, 5), chunked_range=[round(min(ms["chunked"]), 5), round(max(ms["chunked"]), 5)],
                   ratio=round(c / o, 4), model_input_ratio=round((Tc + 2 * L) / Tc, 4),
                   state_bytes_per_stream=int(_lib.lib().ofs_aa_chunk_state_bytes(1, L)),
                   steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(dev))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del one, chk, x, ref, got
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
