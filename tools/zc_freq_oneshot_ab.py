"""The one-shot zc_freq call (ofs_zc_freq_metric on its sliding kernels) of another build of the library
against this tree's, in one process on one device.  Diagnostic for changes that touch csrc/zs_body.h,
csrc/zs_slide_body.h, csrc/zs_pair_body.h or csrc/zc_slide.hip.

    python tools/zc_freq_oneshot_ab.py --other PATH/libofdmsync.so [--out-dir profiles] [--tag zc_freq_chunked]

--other is a libofdmsync.so built from the commit to compare with (check that commit out elsewhere, run
its `python -c 'import __graft_entry__ as g; g.build()'` and pass the library it leaves in
ofdm-sync-math_amd/ofdm_sync_amd/).  Two records are written into --out-dir:

  <tag>_oneshot_dump_compare.txt   the metric of both libraries on the same seeded random streams, compared
      word for word: complex128 with one branch and complex64 with two (f32 out), the PSS template (mirror
      pairs: the pair body) and an unpaired one with the DC bin (the per-bin body), (N, cp, T) = (2048, 512,
      9001), (192, 5, 1400), (8192, 0, 9500), i.e. C = 128 / 64 / 256; 16 streams each.  The tool fails if
      a word differs.
  <tag>_oneshot_parent_ab.jsonl    interleaved timing on the shapes of the zc_freq_fp64 and zc_freq_refshape
      configurations of tools/bench_configs.py: four arms (other_a, new_a, other_b, new_b), order rotated
      over 9 rounds of 40 calls between two events after 30 warm-up calls per arm.  The difference of a
      library's two arms is the A/A spread of this run; new_over_other is to be read against it.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
from ctypes import c_double, c_int32, c_int64, c_void_p as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ofdm-sync-math_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_sync_amd import _lib, zc_freq  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--other", required=True, help="libofdmsync.so of the build to compare with")
ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
ap.add_argument("--tag", default="zc_freq")
args = ap.parse_args()


def load(p):
    l = ctypes.CDLL(os.path.abspath(p))
    l.ofs_zc_freq_metric.restype = c_int32
    l.ofs_zc_freq_metric.argtypes = [c_int32, P, c_int64, c_int32, c_int64, c_int32, c_int32, c_int32, c_int32, P, P,
                                     c_double, P, P]
    return l


libs = [("other", load(args.other)), ("new", load(_lib.LIB_PATH))]
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)
OUT = args.out_dir
os.makedirs(OUT, exist_ok=True)


def tmpl(kind, N):
    idx, tb, te = zc_freq.make_pss_frequency_template()
    if kind == "unpaired":
        rng = np.random.default_rng(5)
        idx = np.arange(0, 41)
        tb = rng.standard_normal(41) + 1j * rng.standard_normal(41)
        te = float(np.sum(np.abs(tb) ** 2))
    return (np.ascontiguousarray(np.asarray(idx, np.int32)), np.ascontiguousarray(np.asarray(tb, np.complex128)), float(te))

def call(l, x, fmt, prec, nb, T, N, cp, t, out):
    rc = l.ofs_zc_freq_metric(fmt, x.data_ptr(), x.shape[0], nb, T, N, cp, prec, int(t[0].size), t[0].ctypes.data,
                              t[1].ctypes.data, t[2], out.data_ptr(), st.cuda_stream)
    assert rc == 0, rc

lines = []
for name, dt, fmt, prec, rdt, nb in (("c128", torch.complex128, _lib.C128, _lib.FP64, torch.float64, 1),
                                     ("c64", torch.complex64, _lib.C64, _lib.FP32, torch.float32, 2)):
    for kind in ("paired", "unpaired"):
        for (N, cp, T) in ((2048, 512, 9001), (192, 5, 1400), (8192, 0, 9500)):
            B = 16
            g = torch.Generator(device=dev).manual_seed(N + nb)
            x = torch.randn((B, nb, T), dtype=dt, device=dev, generator=g)
            t = tmpl(kind, N)
            outs = []
            for ln, l in libs:
                o = torch.full((B, T - N - cp + 1), float("nan"), dtype=rdt, device=dev)
                call(l, x, fmt, prec, nb, T, N, cp, t, o)
                torch.cuda.synchronize()
                outs.append(o.view(torch.int32 if rdt == torch.float32 else torch.int64))
            ndiff = int((outs[0] != outs[1]).sum())
            lines.append(f"{name} n_br={nb} template={kind} N={N} cp={cp} T={T} B={B}: words={outs[0].numel()} differing={ndiff}")
            print(lines[-1], flush=True)
open(os.path.join(OUT, args.tag + "_oneshot_dump_compare.txt"), "w").write("\n".join(lines) + "\n")
assert all(l.endswith("differing=0") for l in lines)

def timed(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(steps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps

rows = []
for cfg, dt, fmt, prec, rdt, B, nb, T in (("zc_freq_fp64", torch.complex128, _lib.C128, _lib.FP64, torch.float64, 256, 1, 16384),
                                          ("zc_freq_refshape", torch.complex64, _lib.C64, _lib.FP32, torch.float32, 4096, 2, 4242)):
    N, cp = 2048, 512
    g = torch.Generator(device=dev).manual_seed(6)
    x = torch.randn((B, nb, T), dtype=dt, device=dev, generator=g)
    t = tmpl("paired", N)
    o = torch.empty((B, T - N - cp + 1), dtype=rdt, device=dev)
    arms = [(ln + s, l) for ln, l in libs for s in ("_a", "_b")]
    arms = [arms[0], arms[2], arms[1], arms[3]]          # other_a, new_a, other_b, new_b
    ms = {n: [] for n, _ in arms}
    for n, l in arms:
        timed(lambda: call(l, x, fmt, prec, nb, T, N, cp, t, o), 30)
    for r in range(9):
        for n, l in arms[r % 4:] + arms[:r % 4]:
            ms[n].append(timed(lambda: call(l, x, fmt, prec, nb, T, N, cp, t, o), 40))
    med = {n: statistics.median(v) for n, v in ms.items()}
    par, new = 0.5 * (med["other_a"] + med["other_b"]), 0.5 * (med["new_a"] + med["new_b"])
    row = dict(tool="zc_freq_oneshot_ab", config=cfg, shape=[B, nb, T, N, cp],
               other_ms=round(par, 5), new_ms=round(new, 5), new_over_other=round(new / par, 5),
               aa_spread_other=round(abs(med["other_a"] - med["other_b"]) / par, 5),
               aa_spread_new=round(abs(med["new_a"] - med["new_b"]) / new, 5),
               ms_all={n: [round(v, 5) for v in vs] for n, vs in ms.items()}, device=torch.cuda.get_device_name(dev))
    rows.append(row)
    print(json.dumps(row), flush=True)
with open(os.path.join(OUT, args.tag + "_oneshot_parent_ab.jsonl"), "w") as fh:
    for r in rows:
        fh.write(json.dumps(r) + "\n")
