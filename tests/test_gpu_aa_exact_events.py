"""GPU: every [A][A] kernel form reproduces the oracle's gate and peak decisions EXACTLY on the
exact-arithmetic streams of tests/exact_streams.py.

On those streams every product, window sum and |P|^2 is a small integer, so fp32 and fp64 agree in any
summation order, no metric lies within 1e-4 of the threshold, and many gates hold exact ties of
|P|^2.  One rule for every path, always against ofdm_oracle.aa_detect on the same stream and without
oracle/parity.py's near-tie exemptions: the event count (also above max_events), the event integers,
P at the peak, stored P and R and valid are EQUAL; cfo_hz is within 1e-6 rad * fs / (2 pi L) without
wrapping (a -pi for the oracle's +pi fails); M at the peak and stored M are within the project's
bounds (1e-6 on fp32 paths, 1e-12 on fp64 paths).  Each case asserts first that the intended kernel
serves it (ofs_aa_plan, or the variant it sets), and prints the largest |M - M_o| and CFO difference.
Every path runs every hysteresis of exact_streams.hysts(T): 0, 1, 2, 16, RL - 1, RL, RL + 1 for the
row lengths 128, 256 and 512, and one value above T.
"""
import numpy as np
import pytest
import torch

import exact_streams as X
from ofdm_sync_amd import _lib, sync_aa, wire

pytestmark = pytest.mark.gpu

E = X.MAX_EVENTS
WORST = {"fp32": [0.0, 0.0], "fp64": [0.0, 0.0]}         # max |dM|, max |dCFO| in rad, per precision


def launch(fmt, x, B, n_ant, T, L, prec, hyst, want=("P", "R", "M"), max_ev=E, flags=None):
    """One ofs_aa_detect(_ex) call on the device batch x; outputs as host arrays.  P and M start as
    zeros (a head-resident call leaves n < L alone), the event slots as -1."""
    dev = x.device
    ct, rt = (torch.complex128, torch.float64) if prec == _lib.FP64 else (torch.complex64, torch.float32)
    out = {k: torch.zeros((B, T), dtype=dt, device=dev)
           for k, dt in (("P", ct), ("R", rt), ("M", rt), ("valid", torch.uint8)) if k in want}
    n_ev = torch.zeros(B, dtype=torch.int32, device=dev)
    ev_i = torch.full((B, max(max_ev, 1), 4), -1, dtype=torch.int64, device=dev)
    ev_r = torch.full((B, max(max_ev, 1), 4), -1.0, dtype=torch.float64, device=dev)
    p = lambda k: out[k].data_ptr() if k in out else None  # noqa: E731
    args = (fmt, x.data_ptr(), B, n_ant, T, L, prec, p("P"), p("R"), p("M"), p("valid"), 1, X.THR, hyst, X.FS,
            max_ev, n_ev.data_ptr(), ev_i.data_ptr(), ev_r.data_ptr(), torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().ofs_aa_detect(*args) if flags is None else _lib.lib().ofs_aa_detect_ex(*args, flags)
    assert rc == 0, rc
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(n_events=n_ev.cpu().numpy(), ev_int=ev_i.cpu().numpy(), ev_real=ev_r.cpu().numpy())
    return res


def compare(res, L, T, hyst, n_ant, fp64, what, max_ev=E):
    """The one comparison rule (module docstring)."""
    names, _ = X.streams(L, T, hyst, n_ant)
    orc = X.oracle(L, T, hyst, n_ant)
    tol_m = 1e-12 if fp64 else 1e-6
    tol_cfo = 1e-6 * X.FS / (2 * np.pi * L)
    dm = dc = 0.0
    for b, name in enumerate(names):
        P, R, M, valid, ei, er = orc[b]
        tag = (what, L, T, hyst, n_ant, name)
        assert res["n_events"][b] == len(ei), (tag, res["n_events"][b], len(ei))
        k = min(len(ei), max_ev)
        assert np.array_equal(res["ev_int"][b, :k], ei[:k]), (tag, res["ev_int"][b, :k].tolist(), ei[:k].tolist())
        gr = res["ev_real"][b, :k]
        assert np.array_equal(gr[:, :2], er[:k, :2]), (tag, gr[:, :2].tolist(), er[:k, :2].tolist())
        if k:
            dm = max(dm, float(np.max(np.abs(gr[:, 2] - er[:k, 2]))))
            dc = max(dc, float(np.max(np.abs(gr[:, 3] - er[:k, 3]))))           # no wrapping
        if "P" in res:
            assert np.array_equal(res["P"][b].astype(np.complex128), P), tag
        if "R" in res:
            assert np.array_equal(res["R"][b].astype(np.float64), R), tag
        if "M" in res:
            dm = max(dm, float(np.max(np.abs(res["M"][b].astype(np.float64) - M), initial=0)))
        if "valid" in res:
            assert np.array_equal(res["valid"][b].astype(bool), valid), tag
        assert dm <= tol_m and dc <= tol_cfo, (tag, dm, dc / tol_cfo * 1e-6)
    w = WORST["fp64" if fp64 else "fp32"]
    w[0], w[1] = max(w[0], dm), max(w[1], dc * 2 * np.pi * L / X.FS)
    return dm, dc * 2 * np.pi * L / X.FS


def report(what, L, T, n_ant, worst):
    print(f"{what} L={L} T={T} n_ant={n_ant}: max |M - M_o| = {worst[0]:.3e}, max CFO difference = {worst[1]:.3e} rad")


def device_c64(L, T, hyst, n_ant):
    _, iq = X.streams(L, T, hyst, n_ant)
    return torch.from_numpy(X.cplx(iq, np.complex64)).cuda(), iq.shape[0]


def plan(fmt, prec, n_ant, T, L):
    return int(_lib.lib().ofs_aa_plan(fmt, prec, n_ant, T, L))


def sweep(L, T, n_ant, arms, what, fmt=_lib.C64, prec=_lib.FP32, make=device_c64):
    """Every hysteresis x every arm (name, variants, launch keywords); the first arm also with one
    event slot (counts above max_events stay exact)."""
    worst = [0.0, 0.0]
    for hyst in X.hysts(T):
        x, B = make(L, T, hyst, n_ant)
        for i, (name, var, kw) in enumerate(arms):
            for max_ev in ((E, 1) if i == 0 else (E,)):
                with _lib.variants(**var):
                    res = launch(fmt, x, B, n_ant, T, L, prec, hyst, max_ev=max_ev, **kw)
                dm, dc = compare(res, L, T, hyst, n_ant, prec == _lib.FP64, (what, name), max_ev)
                worst = [max(worst[0], dm), max(worst[1], dc)]
    report(what, L, T, n_ant, worst)


@pytest.mark.parametrize("L,T,n_ant", X.SHAPES["fast"], ids=str)
def test_register_staged_storing(L, T, n_ant):
    """complex64 / fp32, one antenna, T = 1024: the full-stream form (FS 1 for max(hyst, 1) >= 128,
    FS 2 below), the generic form, E = 4 and 8, fp32 row scans, the resident head, and valid."""
    assert plan(_lib.C64, _lib.FP32, 1, T, L) == 1020 + L // 128
    arms = [("default", {}, {}), ("generic", {"FAST_FULL": 0}, {}), ("scan32", {"FAST_SCAN": 32}, {}),
            ("head", {}, {"flags": _lib.AA_HEAD_RESIDENT}), ("head generic", {"FAST_FULL": 0}, {"flags": _lib.AA_HEAD_RESIDENT}),
            ("valid", {}, {"want": ("P", "R", "M", "valid")}), ("events and M", {}, {"want": ("M",)})]
    for e in (4, 8):
        if L % (64 * e) == 0:
            arms.append((f"E={e}", {"FAST_E": e}, {}))
            with _lib.variants(FAST_E=e):
                assert plan(_lib.C64, _lib.FP32, 1, T, L) == 1000 + 10 * e + L // (64 * e)
    sweep(L, T, n_ant, arms, "register-staged")


@pytest.mark.parametrize("L,T,n_ant", X.SHAPES["short"], ids=str)
def test_register_staged_short_streams(L, T, n_ant):
    """Even T < 1024: the generic row guards (at 1022 the last lane's samples lie beyond T)."""
    assert plan(_lib.C64, _lib.FP32, 1, T, L) == 1020 + L // 128
    arms = [("default", {}, {}), ("head", {}, {"flags": _lib.AA_HEAD_RESIDENT}), ("scan32", {"FAST_SCAN": 32}, {}),
            ("detect-only", {}, {"want": ()})]
    if L % 256 == 0:
        arms.append(("E=4", {"FAST_E": 4}, {}))
    sweep(L, T, n_ant, arms, "short")


@pytest.mark.parametrize("L,T,n_ant", X.SHAPES["fast"] + X.SHAPES["two"][:3], ids=str)
def test_detect_only(L, T, n_ant):
    """No output arrays: E = 4 with fp32 scans by default, E = 2 and 8, fp64 scans."""
    assert 1000 < plan(_lib.C64, _lib.FP32, n_ant, T, L) < 1100
    arms = [("default", {}, {"want": ()}), ("E=2", {"FAST_E_DO": 2}, {"want": ()}),
            ("scan64", {"FAST_SCAN_DO": 64}, {"want": ()})]
    if L % 512 == 0:
        arms.append(("E=8", {"FAST_E_DO": 8}, {"want": ()}))
    sweep(L, T, n_ant, arms, "detect-only")


@pytest.mark.parametrize("L,T,n_ant", X.SHAPES["two"], ids=str)
def test_two_antennas(L, T, n_ant):
    assert plan(_lib.C64, _lib.FP32, 2, T, L) == 1020 + L // 128
    arms = [("default", {}, {}), ("scan32", {"FAST_SCAN": 32}, {}), ("valid", {}, {"want": ("P", "R", "M", "valid")})]
    sweep(L, T, n_ant, arms, "two antennas")


@pytest.mark.parametrize("L,T,n_ant", X.SHAPES["stream"], ids=str)
def test_streaming_kernels(L, T, n_ant):
    """Plans 1121 / 1122 / 1124 / 1128 (E = 2, windows of 1, 2, 4, 8 rows), storing and detect-only."""
    assert plan(_lib.C64, _lib.FP32, n_ant, T, L) == 1120 + L // 128
    arms = [("default", {}, {}), ("detect-only", {}, {"want": ()}), ("valid", {}, {"want": ("P", "R", "M", "valid")})]
    sweep(L, T, n_ant, arms, "streaming")


def device_i16(L, T, hyst, n_ant):
    _, iq = X.streams(L, T, hyst, n_ant)
    return torch.from_numpy(iq.copy()).cuda(), iq.shape[0]


def device_cp12(L, T, hyst, n_ant):
    _, iq = X.streams(L, T, hyst, n_ant)
    return torch.from_numpy(wire.pack_axis(iq)).cuda(), iq.shape[0]


def device_c128(L, T, hyst, n_ant):
    _, iq = X.streams(L, T, hyst, n_ant)
    return torch.from_numpy(X.cplx(iq)).cuda(), iq.shape[0]


WAVE_SHAPES = X.SHAPES["fast"] + [(256, 768, 2), (1024, 4096, 2), (128, 1023, 1)]


@pytest.mark.parametrize("L,T,n_ant", WAVE_SHAPES, ids=str)
def test_integer_exact_wave_kernels(L, T, n_ant):
    """int16 I/Q and packed 12-bit words -> plans 2xxx; EXACT = 0 sends int16 to the general engine."""
    assert plan(_lib.CI16, _lib.FP64, n_ant, T, L) == 2020 + L // 128
    assert plan(_lib.CP12, _lib.FP64, n_ant, T, L) == 2020 + L // 128
    full = {"want": ("P", "R", "M", "valid")}
    sweep(L, T, n_ant, [("int16", {}, full), ("detect-only", {}, {"want": ()})], "int16 wave", _lib.CI16, _lib.FP64,
          device_i16)
    sweep(L, T, n_ant, [("cp12", {}, full)], "cp12 wave", _lib.CP12, _lib.FP64, device_cp12)
    if T <= 1024:
        with _lib.variants(EXACT=0):
            assert plan(_lib.CI16, _lib.FP64, n_ant, T, L) == 1
        sweep(L, T, n_ant, [("EXACT=0", {"EXACT": 0}, full)], "int16 general engine", _lib.CI16, _lib.FP64, device_i16)


@pytest.mark.parametrize("L,T,n_ant", WAVE_SHAPES[:4] + WAVE_SHAPES[5:], ids=str)
def test_complex128_wave_kernels(L, T, n_ant):
    assert plan(_lib.C128, _lib.FP64, n_ant, T, L) == 3020 + L // 128
    sweep(L, T, n_ant, [("complex128", {}, {"want": ("P", "R", "M", "valid")}), ("detect-only", {}, {"want": ()})],
          "complex128 wave", _lib.C128, _lib.FP64, device_c128)


def test_general_engine():
    """L = 192 is served by the general LDS engine: fused (plan 1) in fp32 and fp64, and tiled with
    aa_events_kernel (plan 2) at the smallest T for which ofs_aa_plan says so."""
    L = 192
    full = {"want": ("P", "R", "M", "valid")}
    assert plan(_lib.C64, _lib.FP32, 1, 1024, L) == 1 and plan(_lib.C128, _lib.FP64, 1, 1024, L) == 1
    sweep(L, 1024, 1, [("fused fp32", {}, full), ("detect-only", {}, {"want": ()})], "general fused fp32")
    sweep(L, 1024, 1, [("fused fp64", {}, full)], "general fused fp64", _lib.C128, _lib.FP64, device_c128)
    for fmt, prec, make, name in ((_lib.C64, _lib.FP32, device_c64, "fp32"), (_lib.C128, _lib.FP64, device_c128, "fp64")):
        T = next(t for t in range(L + 1, 1 << 16) if plan(fmt, prec, 1, t, L) == 2)
        assert (L, T, 1) in X.SHAPES["general"], T           # the host test covers this stream set
        assert plan(fmt, prec, 1, T - 1, L) == 1
        sweep(L, T, 1, [("tiled " + name, {}, full)], "general tiled " + name, fmt, prec, make)


def chunkings(T):
    out = [[T]]
    for c in (127, 128, 129, 1000):
        out.append([c] * (T // c) + ([T % c] if T % c else []))
    return out


@pytest.mark.parametrize("L,T,n_ant", X.SHAPES["chunk"], ids=str)
@pytest.mark.parametrize("cp12", [False, True], ids=["int16", "cp12"])
def test_chunked_detector(L, T, n_ant, cp12):
    """AAChunkedDetector (aa_chunk_kernel, the ABS form of the gate machine): the events of any
    chunking, with absolute indices, and the concatenated P, R, M, valid equal the oracle's.  The
    shortest stream is also pushed one sample at a time."""
    worst = [0.0, 0.0]
    for hyst in X.hysts(T):
        names, iq = X.streams(L, T, hyst, n_ant)
        B = len(names)
        nmax = max(len(o[4]) for o in X.oracle(L, T, hyst, n_ant))
        xd = torch.from_numpy(wire.pack_axis(iq) if cp12 else iq.copy()).cuda()
        det = sync_aa.AAChunkedDetector(B, n_ant, L, threshold=X.THR, hysteresis=hyst, sample_rate=X.FS,
                                        in_dtype="cp12" if cp12 else torch.int16,
                                        outputs=("P", "R", "M", "valid"), max_events=max(nmax, 1))
        splits = chunkings(T) + ([[1] * T] if T < 500 and hyst in (0, 16, 128, 257) else [])
        for chunks in splits:
            parts, s = [], 0
            for i, c in enumerate(chunks):
                piece = xd[:, s:s + c] if cp12 else xd[:, :, s:s + c]
                r = det.push(piece.contiguous(), final=i == len(chunks) - 1)
                parts.append([t.clone() for t in (r.P, r.R, r.M, r.valid, r.n_events, r.ev_int, r.ev_real)])
                s += c
            torch.cuda.synchronize()
            res = {k: torch.cat([p[j] for p in parts], dim=1).cpu().numpy() for j, k in enumerate(("P", "R", "M", "valid"))}
            n = np.stack([p[4].cpu().numpy() for p in parts])                  # [pieces, B]
            ev_i = np.full((B, max(nmax, 1), 4), -1, np.int64)
            ev_r = np.full((B, max(nmax, 1), 4), -1.0)
            fill = np.zeros(B, int)
            for j in np.flatnonzero(n.sum(1)):                                 # the pushes that closed a gate
                pi, pr = parts[j][5].cpu().numpy(), parts[j][6].cpu().numpy()
                for b in np.flatnonzero(n[j]):
                    m = int(n[j, b])
                    assert fill[b] + m <= max(nmax, 1), (names[b], hyst, chunks[:3])
                    ev_i[b, fill[b]:fill[b] + m], ev_r[b, fill[b]:fill[b] + m] = pi[b, :m], pr[b, :m]
                    fill[b] += m
            res.update(n_events=n.sum(0), ev_int=ev_i, ev_real=ev_r)
            dm, dc = compare(res, L, T, hyst, n_ant, True, ("chunked", chunks[0], len(chunks)), max(nmax, 1))
            worst = [max(worst[0], dm), max(worst[1], dc)]
    report("chunked " + ("cp12" if cp12 else "int16"), L, T, n_ant, worst)


def test_zz_report_worst():
    """The largest differences this file saw (DESIGN.md records them)."""
    for k, (dm, dc) in WORST.items():
        print(f"exact streams, {k} paths: max |M - M_o| = {dm:.3e}, max unwrapped CFO difference = {dc:.3e} rad")
    assert WORST["fp32"][0] <= 1e-6 and WORST["fp64"][0] <= 1e-12
    assert max(WORST["fp32"][1], WORST["fp64"][1]) <= 1e-6
