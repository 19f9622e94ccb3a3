"""Paired timing of the resumable chunked complex64 [A][A] detector (AAChunkedDetectorF32.push,
ofs_aa_detect_chunk_f32) against the one-shot AABatchDetector: k pushes of Tc samples against ONE
one-shot call on the same k * Tc samples (complex64 in, fp32 out, P / R / M stored, events on), one
build, one process (B = 4096, one antenna, L = 512).  State form (a): a push reads the history
(2L + n_seen % 128 samples), replays L of them and writes the next history, so the model is a ratio
near (Tc + 2L + 128) / Tc on the input / compute side with equal output stores.  A record, not a gate.

    python tools/aa_chunk_f32_ab.py [--B 4096 --L 512 --Tc 1024,4096,16384 --k 4] [--out profiles/aa_chunked_f32_ab.jsonl]

Three arms per round, order rotating: the one-shot call twice (arms a and b: their difference is the
A/A spread of this run) and the k pushes.  Each round times `--steps` repetitions between two events.
The chunked outputs of the first pass on fresh streams are checked bit for bit against the one-shot
P / R / M and events before anything is timed.  The chunked arm reuses one [B, Tc] output buffer per
push (the detector's), the one-shot arm writes [B, k * Tc]: the bytes stored are the same, the
footprint is not.
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

from ofdm_sync_amd import _lib, sync_aa, synth  # noqa: E402
from chunk_ab_common import bits, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--Tc", default="1024,4096,16384")
    ap.add_argument("--k", type=int, default=4, help="pushes per one-shot call")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append one JSON line per Tc to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    B, L, k = a.B, a.L, a.k
    rows = []
    for Tc in [int(v) for v in a.Tc.split(",")]:
        T = k * Tc
        x = synth.make_aa_batch(B, T, L, seed=7, device=dev)
        one = sync_aa.AABatchDetector(B, T, 1, L, placement="plain", rewrite_head=True)
        chk = sync_aa.AAChunkedDetectorF32(B, 1, L)
        pieces = [x[:, :, i * Tc:(i + 1) * Tc].contiguous() for i in range(k)]

        def pushes():
            for i, p in enumerate(pieces):
                chk.push(p, final=i == k - 1)

        ref = one.run(x)
        n_ref = ref.n_events.clone()
        n_got = torch.zeros_like(n_ref)
        for i, p in enumerate(pieces):
            got = chk.push(p, final=i == k - 1)
            for name in ("P", "R", "M"):
                want = getattr(ref, name)[:, i * Tc:(i + 1) * Tc]
                assert torch.equal(bits(getattr(got, name)), bits(want)), f"Tc={Tc}, push {i}: {name} differs"
            n_got += got.n_events
        torch.cuda.synchronize()
        assert torch.equal(n_got, n_ref), f"Tc={Tc}: event counts differ from the one-shot call"
        arms = [("one_shot_a", lambda: one.run(x)), ("chunked", pushes), ("one_shot_b", lambda: one.run(x))]
        ms = {n: [] for n, _ in arms}
        for _, fn in arms:
            timed(fn, a.warmup, st)
        for r in range(a.rounds):
            for name, fn in arms[r % 3:] + arms[:r % 3]:
                ms[name].append(timed(fn, a.steps, st))
        oa, ob, c = (statistics.median(ms[n]) for n in ("one_shot_a", "one_shot_b", "chunked"))
        o = 0.5 * (oa + ob)
        rng = lambda v: [round(min(v), 5), round(max(v), 5)]  # noqa: E731
        row = dict(tool="aa_chunk_f32_ab", B=B, L=L, Tc=Tc, k=k, in_fmt="complex64", precision="fp32",
                   plan_one_shot=one.plan(), one_shot_ms=round(o, 5), one_shot_a_ms=round(oa, 5),
                   one_shot_b_ms=round(ob, 5), one_shot_a_range=rng(ms["one_shot_a"]), one_shot_b_range=rng(ms["one_shot_b"]),
                   aa_spread=round(abs(oa - ob) / o, 5), chunked_ms=round(c, 5), chunked_range=rng(ms["chunked"]),
                   ratio=round(c / o, 4), model_input_ratio=round((Tc + 2 * L + 128) / Tc, 4),
                   state_bytes_per_stream=int(_lib.lib().ofs_aa_chunk_f32_state_bytes(1, L)),
                   steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(dev))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del one, chk, x, ref, got, pieces
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
