"""Paired A/B of libofdmsync.so variants (tools/variants.py) on the same device buffers: the
sync_aa detector (ofs_aa_detect) on one shape, lib order rotated every round.  Diagnostic only.

    python tools/lib_ab.py --libs build/libofdmsync_a.so,build/libofdmsync_b.so --B 65536 --T 4096 --L 512 --na 1
    python tools/lib_ab.py --op zc --libs PARENT/libofdmsync.so,NEW/libofdmsync.so --B 4096 --T 16384 --L 512
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ofdm-sync-math_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ofdm_sync_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True)
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--T", type=int, default=4096)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--na", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--detect-only", action="store_true")
    ap.add_argument("--head-resident", action="store_true",
                    help="aa: P/M heads zeroed once, calls through ofs_aa_detect_ex with OFS_AA_HEAD_RESIDENT")
    ap.add_argument("--no-check", action="store_true", help="variants may differ in rounding (no bit-equality check)")
    ap.add_argument("--op", choices=("aa", "scminn", "sc", "comb", "minn", "zcfreq", "zc"), default="aa",
                    help="aa: ofs_aa_detect; scminn: ofs_sc_minn_metric (cfg4 fused S&C + Minn, N = 2 L); zcfreq: "
                         "ofs_zc_freq_metric on c64 -> f32 (--na branches, N = 4 L, cp = L, the ZC template); zc: "
                         "ofs_zc_detect on every fused plan and ofs_zc_detect_chunk (W = 4 L, hysteresis L / 2)")
    a = ap.parse_args()
    if a.op == "zc":
        return zc(a)
    if a.op == "zcfreq":
        return zcfreq(a)
    if a.op != "aa":
        return scminn(a)
    dev = torch.device("cuda", 0)
    B, T, L, na, E = a.B, a.T, a.L, a.na, 4
    base = synth.faded_base(L, "cir1", tuple(range(na)) if na > 1 else (1,))
    x = synth.synth_batch(base, B, T, seed=5, device=dev)
    P = None if a.detect_only else torch.empty((B, T), dtype=torch.complex64, device=dev)
    R = None if a.detect_only else torch.empty((B, T), dtype=torch.float32, device=dev)
    M = None if a.detect_only else torch.empty((B, T), dtype=torch.float32, device=dev)
    if a.head_resident and not a.detect_only:
        P[:, :min(L, T)].zero_()
        M[:, :min(L, T)].zero_()
    n_ev = torch.zeros(B, dtype=torch.int32, device=dev)
    ev_i = torch.zeros((B, E, 4), dtype=torch.int64, device=dev)       # records past n_ev are never written
    ev_r = torch.zeros((B, E, 4), dtype=torch.float64, device=dev)
    # every output compared bit for bit between the libraries (the stored ones)
    outs = {k: v for k, v in dict(n_ev=n_ev, ev_i=ev_i, ev_r=ev_r, P=P, R=R, M=M).items() if v is not None}
    bits = lambda t: torch.view_as_real(t).view(torch.int32) if t.is_complex() else t.view(
        torch.int64 if t.element_size() == 8 else torch.int32)
    st = torch.cuda.current_stream(dev)
    libs = []
    for p in a.libs.split(","):
        l = ctypes.CDLL(os.path.abspath(p))
        _lib._declare(l)
        libs.append((os.path.basename(p), l))
    args = (_lib.C64, x.data_ptr(), B, na, T, L, _lib.FP32, _lib.ptr(P), _lib.ptr(R), _lib.ptr(M), None, 1,
            0.15, 128, 15.36e6, E, n_ev.data_ptr(), ev_i.data_ptr(), ev_r.data_ptr(), st.cuda_stream)
    run = (lambda l: l.ofs_aa_detect_ex(*args, _lib.AA_HEAD_RESIDENT)) if a.head_resident else (
        lambda l: l.ofs_aa_detect(*args))
    times = {n: [] for n, _ in libs}
    ref = None
    for r in range(a.rounds):
        order = libs[r % len(libs):] + libs[:r % len(libs)]
        for name, l in order:
            for _ in range(3):
                assert run(l) == 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.steps):
                run(l)
            e1.record(st)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
            if ref is None:
                ref = {k: bits(v).clone() for k, v in outs.items()}
            elif not a.no_check:
                for k, v in outs.items():
                    assert torch.equal(ref[k], bits(v)), f"{name}: {k} differs"
    alg = B * T * (na * 8 + (0 if a.detect_only else 16))
    for name, _ in libs:
        ms = statistics.median(times[name])
        print(json.dumps(dict(lib=name, shape=[B, na, T, L], plan=libs[0][1].ofs_aa_plan(_lib.C64, _lib.FP32, na, T, L),
                              head_resident=a.head_resident, ms_median=round(ms, 4), ms_all=[round(t, 4) for t in times[name]],
                              frac=round(alg / (ms / 1e3) / 8e12, 4))), flush=True)


def scminn(a):
    dev = torch.device("cuda", 0)
    B, T, N, nb = a.B, a.T, 2 * a.L, a.na
    x = synth.synth_batch(synth.faded_base(a.L, "cir1", tuple(range(nb)) if nb > 1 else (1,)), B, T, seed=4, device=dev)
    nout = T - N + 1
    n_sets = 2 if a.op == "scminn" else 1
    outs = [torch.empty((B, nout), dtype=dt, device=dev) for dt in (torch.float32, torch.complex64, torch.float32) * n_sets]
    st = torch.cuda.current_stream(dev)
    libs = []
    for p in a.libs.split(","):
        l = ctypes.CDLL(os.path.abspath(p))
        _lib._declare(l)
        libs.append((os.path.basename(p), l))
    optr = [o.data_ptr() for o in outs]
    if a.op == "scminn":
        call = lambda l: l.ofs_sc_minn_metric(_lib.C64, x.data_ptr(), B, nb, T, N, _lib.FP32, *optr, st.cuda_stream)
    elif a.op == "minn":
        call = lambda l: l.ofs_minn_metric(_lib.C64, x.data_ptr(), B, nb, T, N, _lib.FP32, *optr, st.cuda_stream)
    else:
        rm = 0 if a.op == "sc" else 1
        call = lambda l: l.ofs_sc_metric(_lib.C64, x.data_ptr(), B, nb, T, N, rm, _lib.FP32, *optr, st.cuda_stream)
    times = {n: [] for n, _ in libs}
    ref = None
    for r in range(a.rounds):
        for name, l in libs[r % len(libs):] + libs[:r % len(libs)]:
            if not a.no_check:                     # every output element must be rewritten
                for o in outs:
                    o.fill_(float("nan"))
            for _ in range(3):
                assert call(l) == 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.steps):
                call(l)
            e1.record(st)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
            if ref is None:
                ref = [o.clone() for o in outs]
            elif not a.no_check:
                for o, q in zip(outs, ref):
                    assert torch.equal(o, q), f"{name}: outputs differ"
    alg = B * T * 8 * nb + n_sets * B * nout * 16
    for name, _ in libs:
        ms = statistics.median(times[name])
        print(json.dumps(dict(lib=name, op=a.op, shape=[B, nb, T, N], ms_median=round(ms, 4),
                              ms_all=[round(t, 4) for t in times[name]], frac=round(alg / (ms / 1e3) / 8e12, 4))),
              flush=True)


def zcfreq(a):
    """zc_freq on the reference's stream shape by default (--B 4096 --na 2 --T 4242 --L 512: N 2048,
    cp 512); outputs compared within 1e-12 relative (libraries may order the row sums differently)."""
    from ofdm_sync_amd import zc_freq
    dev = torch.device("cuda", 0)
    B, nb, T, N, cp = a.B, a.na, a.T, 4 * a.L, a.L
    g = torch.Generator(device=dev).manual_seed(8)
    x = torch.randn((B, nb, T), dtype=torch.complex64, device=dev, generator=g)
    idx, tb, e = zc_freq.make_pss_frequency_template()
    idx = np.ascontiguousarray(np.asarray(idx, np.int32))
    tb = np.ascontiguousarray(np.asarray(tb, np.complex128))
    noff = T - (N + cp) + 1
    out = torch.empty((B, noff), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev)
    libs = []
    for p in a.libs.split(","):
        l = ctypes.CDLL(os.path.abspath(p))
        _lib._declare(l)
        libs.append((os.path.basename(p), l))
    call = lambda l: l.ofs_zc_freq_metric(_lib.C64, x.data_ptr(), B, nb, T, N, cp, _lib.FP32, int(idx.size),
                                          idx.ctypes.data, tb.ctypes.data, float(e), out.data_ptr(), st.cuda_stream)
    times = {n: [] for n, _ in libs}
    ref = None
    for r in range(a.rounds):
        for name, l in libs[r % len(libs):] + libs[:r % len(libs)]:
            out.fill_(float("nan"))
            for _ in range(3):
                assert call(l) == 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(a.steps):
                call(l)
            e1.record(st)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
            if ref is None:
                ref = out.double().clone()
            elif not a.no_check:
                d = ((out.double() - ref).abs() / ref.abs().clamp_min(1e-30)).max().item()
                assert d <= 1e-6, f"{name}: metric differs by {d:.3g} relative"
    for name, _ in libs:
        ms = statistics.median(times[name])
        print(json.dumps(dict(lib=name, op=a.op, shape=[B, nb, T, N, cp], ms_median=round(ms, 4),
                              ms_all=[round(t, 4) for t in times[name]])), flush=True)


def zc(a):
    """zc_v2 CFAR + gate on B x T float64 magnitudes (--B 4096 --T 16384 --L 512: the shape of
    tools/zc_chunk_ab.py): the one-shot call on its three fused plans and the resumable call in three
    pushes, every output poisoned before each library's run and compared bit for bit between them."""
    from zc_chunk_ab import FRAC, MAX_EV, MIN_MAG, REFLEN, make_mag
    dev = torch.device("cuda", 0)
    B, n, W, hyst = a.B, a.T, 4 * a.L, a.L // 2
    tv = int(4.0 * (1 << FRAC) / W)
    mag = make_mag(B, n, dev)
    st = torch.cuda.current_stream(dev)
    libs = []
    for p in a.libs.split(","):
        l = ctypes.CDLL(os.path.abspath(p))
        _lib._declare(l)
        libs.append((p, l))                                      # the path as given: in-tree libraries share a file name
    f64, u8 = torch.float64, torch.uint8
    cuts = [0, n // 2, n // 2 + n // 4 + 37, n]                   # pushes: a whole number of chunks, an odd one, the rest
    sb = libs[0][1].ofs_zc_chunk_state_bytes(W)
    cases = [("events + mask", {}, False, False), ("state arrays", {}, True, False),
             ("register tiles, state arrays", {"ZC_NODMA": 1}, True, False), ("chunked, state arrays", {}, True, True)]
    for name, var, state, chunked in cases:
        arr = [torch.empty((B, n), dtype=dt, device=dev) if state else None for dt in (f64, f64, f64, u8, u8)]
        gm = torch.empty((B, n), dtype=u8, device=dev)
        n_ev = torch.empty((B,), dtype=torch.int32, device=dev)
        ev = torch.empty((B, MAX_EV, 4), dtype=torch.int64, device=dev)
        pv = torch.empty((B, MAX_EV), dtype=f64, device=dev)
        og = torch.empty((B,), dtype=torch.int64, device=dev)
        stt = torch.zeros((B, sb), dtype=u8, device=dev)
        outs = [t for t in arr if t is not None] + [gm, n_ev, ev, pv, og]
        # a push writes [B][Tc] blocks: one set of buffers per push, copied into the [B][n] arrays afterwards
        blk = [[None if t is None else torch.empty((B, e - b), dtype=t.dtype, device=dev) for t in arr + [gm]]
               for b, e in zip(cuts, cuts[1:])] if chunked else []

        def run(l):
            if not chunked:
                return l.ofs_zc_detect(mag.data_ptr(), B, n, W, tv, FRAC, MIN_MAG, REFLEN, hyst, *[_lib.ptr(t) for t in arr],
                                       gm.data_ptr(), MAX_EV, n_ev.data_ptr(), ev.data_ptr(), pv.data_ptr(), st.cuda_stream)
            rc = 0
            for k, (b, e) in enumerate(zip(cuts, cuts[1:])):
                rc |= l.ofs_zc_detect_chunk(mag.data_ptr() + 8 * b, n, B, e - b, W, tv, FRAC, MIN_MAG, REFLEN, hyst,
                                            stt.data_ptr(), *[_lib.ptr(t) for t in blk[k]], MAX_EV, n_ev.data_ptr(),
                                            ev.data_ptr(), pv.data_ptr(), og.data_ptr(), int(e == n), st.cuda_stream)
            return rc

        times, ref = {nm: [] for nm, _ in libs}, None
        for r in range(a.rounds):
            for nm, l in libs[r % len(libs):] + libs[:r % len(libs)]:
                for k, v in var.items():
                    l.ofs_debug_set_variant(k.encode(), v)
                plan = l.ofs_zc_detect_plan(n, W, hyst, int(state), int(mag.data_ptr() % 16 == 0))
                for t in outs + [t for row in blk for t in row if t is not None]:
                    t.view(u8).fill_(0xA5)                       # every compared byte must be written by this library
                ev.zero_()                                       # records past n_events are never written
                pv.zero_()
                assert run(l) == 0
                torch.cuda.synchronize()
                for k, (b, e) in enumerate(zip(cuts, cuts[1:]) if chunked else ()):
                    for t, part in zip(arr + [gm], blk[k]):
                        if t is not None:
                            t[:, b:e] = part
                got = [t.clone() for t in (outs if chunked else outs[:-1])]   # open_gate_start: the resumable call's
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(a.steps):
                    run(l)
                e1.record(st)
                torch.cuda.synchronize()
                times[nm].append(e0.elapsed_time(e1) / a.steps)
                l.ofs_debug_reset_variants()
                if ref is None:
                    ref = got
                elif not a.no_check:
                    for i, (x, y) in enumerate(zip(ref, got)):
                        assert torch.equal(x.view(u8), y.view(u8)), f"{nm}: {name}: output {i} differs"
        for nm, _ in libs:
            ms = statistics.median(times[nm])
            print(json.dumps(dict(lib=nm, op="zc", case=name, plan=plan, shape=[B, n, W, hyst], ms_median=round(ms, 4),
                                  ms_all=[round(t, 4) for t in times[nm]], bit_equal=not a.no_check,
                                  events_mean=round(float(n_ev.float().mean()), 3))), flush=True)


if __name__ == "__main__":
    main()
