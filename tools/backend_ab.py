"""Paired timing of the receiver back-end between two builds of libofdmsync.so on the same device buffers:
the ``backend`` configuration of tools/bench_configs.py (16384 frames x 2 branches, N = 2048, CP = 512,
1200 used bins, complex64 in), library order rotating every round, one process.  Diagnostic only.

    python tools/backend_ab.py --parent PARENT/libofdmsync.so [--new ofdm-sync-math_amd/ofdm_sync_amd/libofdmsync.so]
                               [--out profiles/backend_origin_ab.jsonl]

Arms: the parent's ofs_rx_backend twice (a and b: their difference is the A/A spread of this run), the new
build's ofs_rx_backend, and the new build's ofs_rx_backend_at with an all-zero origin.  The outputs of
every arm are checked bit for bit against the parent's before anything is timed.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ofdm-sync-math_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_sync_amd import _lib, core  # noqa: E402
from chunk_ab_common import bits, timed  # noqa: E402


class _Signatures:
    """Stands in for a library in ``_lib._declare``: collects (restype, argtypes) per entry point."""

    def __getattr__(self, name):
        fn = types.SimpleNamespace()
        setattr(self, name, fn)
        return fn


def load(path):
    """The library at ``path`` with the two back-end entries declared as ofdm_sync_amd._lib declares them
    (the parent build has no ofs_rx_backend_at, so ``_lib._declare`` itself cannot take it)."""
    sig = _Signatures()
    _lib._declare(sig)
    l = ctypes.CDLL(os.path.abspath(path))
    for name in ("ofs_rx_backend", "ofs_rx_backend_at"):
        fn = getattr(l, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = getattr(sig, name).restype, getattr(sig, name).argtypes
    return l


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", default=_lib.LIB_PATH)
    ap.add_argument("--B", type=int, default=16384)
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--n-used", type=int, default=1200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st = torch.cuda.current_stream(dev)
    old, new = load(a.parent), load(a.new)
    B, N, nb = a.B, a.N, 2
    cp = min(N // 4, 512)
    T = 2 * (N + cp) + 64
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn((B, nb, T), dtype=torch.complex64, device=dev, generator=g)
    k = core.centered_subcarrier_indices(a.n_used)
    U = k.size
    ps = torch.full((B,), 32, dtype=torch.int64, device=dev)
    ds = ps + N + cp
    pil = torch.ones((U,), dtype=torch.complex128, device=dev)
    kb = torch.as_tensor(k.astype(np.int32)).to(dev)
    org = torch.zeros((B,), dtype=torch.int64, device=dev)

    def outputs():
        return ([torch.empty((B,), dtype=torch.float64, device=dev) for _ in range(5)] +
                [torch.empty((B, U), dtype=torch.complex128, device=dev) for _ in range(2)] +
                [torch.empty((B,), dtype=torch.complex128, device=dev)])

    def arm(lib, at, o):
        args = (_lib.C64, x.data_ptr(), B, nb, T, N, cp, 30.72e6, ps.data_ptr(), ds.data_ptr(), None, U, kb.data_ptr(),
                pil.data_ptr(), 0, pil.data_ptr(), 0, o[0].data_ptr(), o[5].data_ptr(), o[6].data_ptr(), o[7].data_ptr(),
                o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr())
        if at:
            return lambda: _lib.check(lib.ofs_rx_backend_at(*args, org.data_ptr(), st.cuda_stream), "ofs_rx_backend_at")
        return lambda: _lib.check(lib.ofs_rx_backend(*args, st.cuda_stream), "ofs_rx_backend")

    o_ref, o_new, o_at = outputs(), outputs(), outputs()
    arms = [("parent_a", arm(old, False, o_ref)), ("new", arm(new, False, o_new)), ("new_at_zero", arm(new, True, o_at)),
            ("parent_b", arm(old, False, o_ref))]
    for _, fn in arms:
        fn()
    torch.cuda.synchronize()
    for o in (o_new, o_at):
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(o_ref, o)), "outputs differ from the parent's"
    ms = {n: [] for n, _ in arms}
    for _, fn in arms:
        timed(fn, a.warmup, st)
    for r in range(a.rounds):
        for name, fn in arms[r % len(arms):] + arms[:r % len(arms)]:
            ms[name].append(timed(fn, a.steps, st))
    med = {n: statistics.median(v) for n, v in ms.items()}
    p = 0.5 * (med["parent_a"] + med["parent_b"])
    row = dict(tool="backend_ab", config="backend", B=B, N=N, cp=cp, n_used=int(U), n_branch=nb, in_fmt="complex64",
               parent_ms=round(p, 5), aa_spread=round(abs(med["parent_a"] - med["parent_b"]) / p, 5),
               new_ratio=round(med["new"] / p, 4), new_at_zero_ratio=round(med["new_at_zero"] / p, 4),
               steps=a.steps, rounds=a.rounds, device=torch.cuda.get_device_name(dev))
    for n, v in ms.items():
        row[n + "_ms"] = round(med[n], 5)
        row[n + "_range"] = [round(min(v), 5), round(max(v), 5)]
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
