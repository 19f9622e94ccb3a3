"""Paired timing of the resumable chunked Park metric (ParkChunkedMetric.push, ofs_park_metric_chunk)
against the one-shot call: k pushes of Tc samples against ONE ofs_park_metric call on the same k * Tc
samples (complex64 in, fp32 out, M / P / E stored, the running peak tracked), one build, one process
(B = 2048, one branch, N = 2048: the shape of the park_fp32 row of DESIGN §7).  A push computes no
output twice; it re-reads the 2 * half + 6 samples before the chunk at most, so the input-side model is
(Tc + 2 * half) / Tc - but the kernel is FMA bound (O(N) multiply-accumulates per output), so the
expectation is a ratio near 1 plus the second, small launch of every push (ring write-back and peak
fold).  The chunked calls also store the 2 * half - 1 zeros of the fill phase and the one output that
the one-shot call on k * Tc samples does not have (d = k * Tc - half; the one-shot call's last is
d = k * Tc - half - 1).  A record, not a gate.

    python tools/park_chunk_ab.py [--B 2048 --N 2048 --Tc 1024,4096,16384 --k 4] [--out profiles/park_chunked_ab.jsonl]

Three arms per round, order rotating: the one-shot call twice (arms a and b: their difference is the
A/A spread of this run) and the k pushes.  Each round times `--steps` repetitions between two events.
The chunked outputs of the first pass on fresh streams are checked bit for bit against the one-shot
M / P / E, and the last peak against ofs_row_argmax of the one-shot M, before anything is timed.  The
chunked arm reuses one [B, Tc] output buffer per push (the object's), the one-shot arm writes
[B, k * Tc - 2 * half].

--phases puts two more arms into the rotation, to see what the model leaves out: ONE push of all k * Tc
samples (the chunked kernels on the one-shot call's own work: no history read) and the k pushes without
the peak (outputs M / P / E, track_peak=False: the second launch only writes the ring).
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

from ofdm_sync_amd import _lib, park, synth  # noqa: E402
from chunk_ab_common import bits, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=2048)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--Tc", default="1024,4096,16384")
    ap.add_argument("--k", type=int, default=4, help="pushes per one-shot call")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--phases", action="store_true",
                    help="two more arms in the rotation: ONE push of all k * Tc samples (no history read) and the "
                         "k pushes without the peak (the second launch only writes the ring)")
    ap.add_argument("--out", default=None, help="append one JSON line per Tc to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    B, N, k = a.B, a.N, a.k
    half = N // 2
    L = _lib.lib()
    rows = []
    for Tc in [int(v) for v in a.Tc.split(",")]:
        T = k * Tc
        assert T >= 2 * half + 1, (T, N)
        x = synth.make_aa_batch(B, T, min(half, 1024), seed=7, device=dev)
        n_out = T - 2 * half
        M = torch.empty((B, n_out), dtype=torch.float32, device=dev)
        P = torch.empty((B, n_out), dtype=torch.complex64, device=dev)
        E = torch.empty((B, n_out), dtype=torch.float32, device=dev)

        def one_shot():
            rc = L.ofs_park_metric(_lib.C64, x.data_ptr(), B, 1, T, N, _lib.FP32, M.data_ptr(), P.data_ptr(),
                                   E.data_ptr(), _lib.stream_ptr())
            _lib.check(rc, "ofs_park_metric")

        chk = park.ParkChunkedMetric(B, 1, N)
        pieces = [x[:, :, i * Tc:(i + 1) * Tc].contiguous() for i in range(k)]

        def pushes():
            for i, p in enumerate(pieces):
                chk.push(p, final=i == k - 1)

        one_shot()
        for i, p in enumerate(pieces):
            got = chk.push(p, final=i == k - 1)
            lo = i * Tc - (2 * half - 1)                     # one-shot index of element 0
            skip = min(max(-lo, 0), Tc)                      # elements of the fill phase (d < half)
            n_cmp = min(Tc, n_out - lo) - skip               # the last push holds one output more
            for name, want in (("M", M), ("P", P), ("E", E)):
                g = bits(getattr(got, name))
                assert not bool(g[:, :skip].any()), f"Tc={Tc}, push {i}: {name} fill is not +0.0"
                assert torch.equal(g[:, skip:skip + n_cmp], bits(want[:, lo + skip:lo + skip + n_cmp])), \
                    f"Tc={Tc}, push {i}: {name} differs"
        idx = torch.empty((B,), dtype=torch.int64, device=dev)
        val = torch.empty((B,), dtype=torch.float64, device=dev)
        _lib.check(L.ofs_row_argmax(_lib.FP32, M.data_ptr(), B, n_out, idx.data_ptr(), val.data_ptr(),
                                    _lib.stream_ptr()), "ofs_row_argmax")
        assert torch.equal(got.peak_index, idx + half) and torch.equal(got.peak_value, val), f"Tc={Tc}: peak differs"
        torch.cuda.synchronize()
        arms = [("one_shot_a", one_shot), ("chunked", pushes), ("one_shot_b", one_shot)]
        if a.phases:
            whole = park.ParkChunkedMetric(B, 1, N)
            plain = park.ParkChunkedMetric(B, 1, N, track_peak=False)

            def plain_pushes():
                for i, p in enumerate(pieces):
                    plain.push(p, final=i == k - 1)

            arms += [("one_push", lambda: whole.push(x, final=True)), ("chunked_no_peak", plain_pushes)]
        ms = {n: [] for n, _ in arms}
        for _, fn in arms:
            timed(fn, a.warmup, st)
        for r in range(a.rounds):
            for name, fn in arms[r % len(arms):] + arms[:r % len(arms)]:
                ms[name].append(timed(fn, a.steps, st))
        oa, ob, c = (statistics.median(ms[n]) for n in ("one_shot_a", "one_shot_b", "chunked"))
        o = 0.5 * (oa + ob)
        rng = lambda v: [round(min(v), 5), round(max(v), 5)]  # noqa: E731
        row = dict(tool="park_chunk_ab", B=B, N=N, n_branch=1, Tc=Tc, k=k, in_fmt="complex64", precision="fp32",
                   one_shot_ms=round(o, 5), one_shot_a_ms=round(oa, 5), one_shot_b_ms=round(ob, 5),
                   one_shot_a_range=rng(ms["one_shot_a"]), one_shot_b_range=rng(ms["one_shot_b"]),
                   aa_spread=round(abs(oa - ob) / o, 5), chunked_ms=round(c, 5), chunked_range=rng(ms["chunked"]),
                   ratio=round(c / o, 4), model_input_ratio=round((Tc + 2 * half) / Tc, 4),
                   outputs_one_shot=n_out, outputs_chunked=T - (2 * half - 1),
                   model_output_ratio=round((T - (2 * half - 1)) / n_out, 4),
                   state_bytes_per_stream=int(L.ofs_park_chunk_state_bytes(_lib.C64, 1, N)),
                   steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(dev))
        for name in ("one_push", "chunked_no_peak"):
            if name in ms:
                row[name + "_ms"] = round(statistics.median(ms[name]), 5)
                row[name + "_range"] = rng(ms[name])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del chk, x, M, P, E, got, pieces, arms
        whole = plain = None
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
