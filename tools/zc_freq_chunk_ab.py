"""Paired timing of the resumable chunked zc_freq metric (FrequencyMetricChunked.push,
ofs_zc_freq_metric_chunk) against the one-shot call: k pushes of Tc samples against ONE
ofs_zc_freq_metric call on the same k * Tc samples, one build, one process.  Two configurations of
B = 256 streams, N = 2048, cp = 512, the PSS template: complex128 in / f64 out with one branch, and the
reference shape's format, complex64 in / f32 out with two branches.

A push starts its first chunk of C offsets from that chunk's own window, as the one-shot call does: it
recomputes the block DFTs of one window (N samples) and replays at most C - 1 steps of the recursion
whose outputs an earlier push stored.  The model for the block and slide work is therefore
(Tc + N + C) / Tc; on top come the second, small launch of every push (ring write-back and peak fold,
which reads the metric row once more) and the N + cp - 1 zeros of the fill phase.  A record, not a gate.

    python tools/zc_freq_chunk_ab.py [--B 256 --N 2048 --cp 512 --Tc 1024,4096,16384 --k 4]
                                     [--out profiles/zc_freq_chunked_ab.jsonl]

Four arms per round, order rotating: the one-shot call twice (arms a and b: their difference is the A/A
spread of this run), the k pushes, and ONE push of all k * Tc samples (the chunked kernels on the
one-shot call's own work: no history read, one write-back).  Each round times `--steps` repetitions
between two events.  The chunked outputs of the first pass on fresh streams are checked bit for bit
against the one-shot metric, and the last peak against ofs_row_argmax of it, before anything is timed.
The chunked arm reuses one [B, Tc] output buffer per push (the object's), the one-shot arm writes
[B, k * Tc - (N + cp) + 1].
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

from ofdm_sync_amd import _lib, zc_freq  # noqa: E402
from chunk_ab_common import bits, timed  # noqa: E402

CONFIGS = (("complex128", torch.complex128, _lib.C128, _lib.FP64, torch.float64, 1),
           ("complex64", torch.complex64, _lib.C64, _lib.FP32, torch.float32, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--cp", type=int, default=512)
    ap.add_argument("--Tc", default="1024,4096,16384")
    ap.add_argument("--k", type=int, default=4, help="pushes per one-shot call")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append one JSON line per configuration and Tc to this file")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    B, N, cp, k = a.B, a.N, a.cp, a.k
    need = N + cp
    L = _lib.lib()
    idx, tb, te = zc_freq.make_pss_frequency_template()
    idx = np.ascontiguousarray(np.asarray(idx, np.int32))
    tb = np.ascontiguousarray(np.asarray(tb, np.complex128))
    rows = []
    for name, dt, fmt, prec, rdt, nb in CONFIGS:
        for Tc in [int(v) for v in a.Tc.split(",")]:
            T = k * Tc
            assert T - need + 1 > 64, (T, N, cp)
            g = torch.Generator(device=dev).manual_seed(11)
            x = torch.randn((B, nb, T), dtype=dt, device=dev, generator=g)
            n_out = T - need + 1
            M = torch.empty((B, n_out), dtype=rdt, device=dev)
            plan = L.ofs_zc_freq_plan(fmt, prec, T, N, cp)
            assert plan in (4, 5), plan

            def one_shot():
                rc = L.ofs_zc_freq_metric(fmt, x.data_ptr(), B, nb, T, N, cp, prec, int(idx.size), idx.ctypes.data,
                                          tb.ctypes.data, float(te), M.data_ptr(), _lib.stream_ptr())
                _lib.check(rc, "ofs_zc_freq_metric")

            chk = zc_freq.FrequencyMetricChunked(B, nb, dtype=dt, N=N, cp=cp)
            whole = zc_freq.FrequencyMetricChunked(B, nb, dtype=dt, N=N, cp=cp)
            pieces = [x[:, :, i * Tc:(i + 1) * Tc].contiguous() for i in range(k)]

            def pushes():
                for i, p in enumerate(pieces):
                    chk.push(p, final=i == k - 1)

            one_shot()
            for i, p in enumerate(pieces):
                got = bits(chk.push(p, final=i == k - 1))
                lo = i * Tc - (need - 1)                         # one-shot index of element 0
                skip = min(max(-lo, 0), Tc)                      # elements of the fill phase (s < 0)
                assert not bool(got[:, :skip].any()), f"{name} Tc={Tc}, push {i}: fill is not +0.0"
                assert torch.equal(got[:, skip:], bits(M[:, lo + skip:lo + Tc])), f"{name} Tc={Tc}, push {i}: differs"
            pi = torch.empty((B,), dtype=torch.int64, device=dev)
            pv = torch.empty((B,), dtype=torch.float64, device=dev)
            _lib.check(L.ofs_row_argmax(prec, M.data_ptr(), B, n_out, pi.data_ptr(), pv.data_ptr(),
                                        _lib.stream_ptr()), "ofs_row_argmax")
            assert torch.equal(chk.peak_index, pi) and torch.equal(chk.peak_value, pv), f"{name} Tc={Tc}: peak differs"
            torch.cuda.synchronize()
            arms = [("one_shot_a", one_shot), ("chunked", pushes), ("one_shot_b", one_shot),
                    ("one_push", lambda: whole.push(x, final=True))]
            ms = {n: [] for n, _ in arms}
            for _, fn in arms:
                timed(fn, a.warmup, st)
            for r in range(a.rounds):
                for arm, fn in arms[r % len(arms):] + arms[:r % len(arms)]:
                    ms[arm].append(timed(fn, a.steps, st))
            oa, ob, c, w = (statistics.median(ms[n]) for n in ("one_shot_a", "one_shot_b", "chunked", "one_push"))
            o = 0.5 * (oa + ob)
            C = (int(L.ofs_zc_freq_chunk_state_bytes(fmt, nb, N, cp)) - 64) // (nb * x.element_size()) - N
            rng = lambda v: [round(min(v), 5), round(max(v), 5)]  # noqa: E731
            row = dict(tool="zc_freq_chunk_ab", B=B, N=N, cp=cp, n_branch=nb, Tc=Tc, k=k, in_fmt=name,
                       precision="fp64" if prec == _lib.FP64 else "fp32", one_shot_plan=int(plan), C=C,
                       one_shot_ms=round(o, 5), one_shot_a_ms=round(oa, 5), one_shot_b_ms=round(ob, 5),
                       one_shot_a_range=rng(ms["one_shot_a"]), one_shot_b_range=rng(ms["one_shot_b"]),
                       aa_spread=round(abs(oa - ob) / o, 5), chunked_ms=round(c, 5), chunked_range=rng(ms["chunked"]),
                       ratio=round(c / o, 4), model_ratio=round((Tc + N + C) / Tc, 4),
                       one_push_ms=round(w, 5), one_push_range=rng(ms["one_push"]), one_push_ratio=round(w / o, 4),
                       outputs_one_shot=n_out, outputs_chunked=T,
                       state_bytes_per_stream=int(L.ofs_zc_freq_chunk_state_bytes(fmt, nb, N, cp)),
                       steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(dev))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del chk, whole, x, M, got, pieces, arms
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
