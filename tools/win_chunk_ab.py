"""Paired timing of the resumable chunked window metrics (WindowMetricChunked.push, ofs_win_metric_chunk)
against the one-shot call: k pushes of Tc samples against ONE ofs_sc_metric / ofs_minn_metric call on the
same k * Tc samples (complex64 in, fp32 out, M / P / R stored), one build, one process (B = 4096, one
branch, N = 2048, kinds 2 = combined S&C and 3 = Minn).  A push reads the history ((HR + 2 MW) rows +
n_seen % RL samples: 1.5 N for kind 2, N for kind 3), replays all but the first MW rows of it and writes
the next history, so the model is a ratio near (Tc + history) / Tc on the input / compute side with
nearly equal output stores (the chunked calls also store the N - 1 zeros of the fill phase).  A record,
not a gate.

    python tools/win_chunk_ab.py [--B 4096 --N 2048 --kinds 2,3 --Tc 1024,4096,16384 --k 4] [--out profiles/win_chunked_ab.jsonl]

Three arms per round, order rotating: the one-shot call twice (arms a and b: their difference is the
A/A spread of this run) and the k pushes.  Each round times `--steps` repetitions between two events.
The chunked outputs of the first pass on fresh streams are checked bit for bit against the one-shot
M / P / R before anything is timed.  The chunked arm reuses one [B, Tc] output buffer per push (the
object's), the one-shot arm writes [B, k * Tc - N + 1].

--phases puts three more arms into the rotation, to see what the input-side model leaves out: ONE push
of all k * Tc samples (the chunked kernel on the one-shot call's own work: no history read, replayed or
written), the k pushes with outputs=() and the one-shot call with null outputs (both without output
stores).  Their medians go into the same row (profiles/win_chunked_phase.jsonl).
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

from ofdm_sync_amd import _lib, _metrics, synth  # noqa: E402
from chunk_ab_common import bits, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--kinds", default="2,3")
    ap.add_argument("--Tc", default="1024,4096,16384")
    ap.add_argument("--k", type=int, default=4, help="pushes per one-shot call")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--phases", action="store_true",
                    help="three more arms in the rotation: ONE push of all k * Tc samples (the chunked kernel on the "
                         "one-shot call's work, no history), the k pushes with outputs=() and the one-shot call "
                         "with null outputs (input, compute and history without the output stores)")
    ap.add_argument("--out", default=None, help="append one JSON line per (kind, Tc) to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    B, N, k = a.B, a.N, a.k
    L = _lib.lib()
    rows = []
    for kind in [int(v) for v in a.kinds.split(",")]:
        for Tc in [int(v) for v in a.Tc.split(",")]:
            T = k * Tc
            plan = int(L.ofs_win_plan(kind, _lib.C64, _lib.FP32, 1, T, N))
            assert plan > 0 and T >= N, (kind, T, N, plan)
            RL, MW = 64 * (plan // 10), plan % 10
            hist = ((0, MW, 2 * MW)[kind - 1] + 2 * MW) * RL + Tc % RL
            x = synth.make_aa_batch(B, T, min(N // 2, 1024), seed=7, device=dev)
            n_out = T - N + 1
            M = torch.empty((B, n_out), dtype=torch.float32, device=dev)
            P = torch.empty((B, n_out), dtype=torch.complex64, device=dev)
            R = torch.empty((B, n_out), dtype=torch.float32, device=dev)

            def one_shot(outs=(M, P, R)):
                ptrs = [_lib.ptr(t) for t in outs]
                if kind == 3:
                    rc = L.ofs_minn_metric(_lib.C64, x.data_ptr(), B, 1, T, N, _lib.FP32, *ptrs, _lib.stream_ptr())
                else:
                    rc = L.ofs_sc_metric(_lib.C64, x.data_ptr(), B, 1, T, N, kind - 1, _lib.FP32, *ptrs,
                                         _lib.stream_ptr())
                _lib.check(rc, "one-shot window metric")

            chk = _metrics.WindowMetricChunked(kind, B, 1, N)
            pieces = [x[:, :, i * Tc:(i + 1) * Tc].contiguous() for i in range(k)]

            def pushes():
                for i, p in enumerate(pieces):
                    chk.push(p, final=i == k - 1)

            one_shot()
            for i, p in enumerate(pieces):
                got = chk.push(p, final=i == k - 1)
                lo = i * Tc - (N - 1)                            # d of element 0
                skip = min(max(-lo, 0), Tc)                      # elements of the fill phase (d < 0)
                for name, want in (("M", M), ("P", P), ("R", R)):
                    g = bits(getattr(got, name))
                    assert not bool(g[:, :skip].any()), f"kind={kind}, Tc={Tc}, push {i}: {name} fill is not +0.0"
                    assert torch.equal(g[:, skip:], bits(want[:, lo + skip:lo + skip + (Tc - skip)])), \
                        f"kind={kind}, Tc={Tc}, push {i}: {name} differs"
            torch.cuda.synchronize()
            arms = [("one_shot_a", one_shot), ("chunked", pushes), ("one_shot_b", one_shot)]
            if a.phases:
                whole = _metrics.WindowMetricChunked(kind, B, 1, N)
                quiet = _metrics.WindowMetricChunked(kind, B, 1, N, outputs=())

                def quiet_pushes():
                    for i, p in enumerate(pieces):
                        quiet.push(p, final=i == k - 1)

                arms += [("one_push", lambda: whole.push(x, final=True)), ("chunked_no_out", quiet_pushes),
                         ("one_shot_no_out", lambda: one_shot((None, None, None)))]
            ms = {n: [] for n, _ in arms}
            for _, fn in arms:
                timed(fn, a.warmup, st)
            for r in range(a.rounds):
                for name, fn in arms[r % len(arms):] + arms[:r % len(arms)]:
                    ms[name].append(timed(fn, a.steps, st))
            oa, ob, c = (statistics.median(ms[n]) for n in ("one_shot_a", "one_shot_b", "chunked"))
            o = 0.5 * (oa + ob)
            rng = lambda v: [round(min(v), 5), round(max(v), 5)]  # noqa: E731
            row = dict(tool="win_chunk_ab", kind=kind, B=B, N=N, n_branch=1, Tc=Tc, k=k, in_fmt="complex64",
                       precision="fp32", plan_one_shot=plan, one_shot_ms=round(o, 5), one_shot_a_ms=round(oa, 5),
                       one_shot_b_ms=round(ob, 5), one_shot_a_range=rng(ms["one_shot_a"]),
                       one_shot_b_range=rng(ms["one_shot_b"]), aa_spread=round(abs(oa - ob) / o, 5),
                       chunked_ms=round(c, 5), chunked_range=rng(ms["chunked"]), ratio=round(c / o, 4),
                       history_samples=hist, model_input_ratio=round((Tc + hist) / Tc, 4),
                       state_bytes_per_stream=int(L.ofs_win_chunk_state_bytes(kind, 1, N)),
                       steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(dev))
            for name in ("one_push", "chunked_no_out", "one_shot_no_out"):
                if name in ms:
                    row[name + "_ms"] = round(statistics.median(ms[name]), 5)
                    row[name + "_range"] = rng(ms[name])
            rows.append(row)
            print(json.dumps(row), flush=True)
            del chk, x, M, P, R, got, pieces, arms
            whole = quiet = None
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
