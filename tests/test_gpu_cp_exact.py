"""GPU: the CP-correlation searches (cp_search_kernel, csrc/cp_search.hip) and the CP CFO (cp_cfo_kernel,
csrc/ofdmsync.hip) reproduce the oracle EXACTLY on the exact streams of tests/cp_streams.py.

Those streams hold small integers, so every window sum, and in robust mode the sum over the range, is exact
in any order and ties are real: plateaus across a lane, a wave and the 256-thread stride, equal maxima on a
thread's second pass and a higher thread's first, axis-aligned ties of different phase, all-zero ranges,
ranges of 1 to 600 offsets clipped at 0 and at T - (N + w), empty ranges, and NaN / Inf samples
(tests/test_cp_streams_host.py proves the facts present and every single wrong decision caught).  One rule,
always against ofdm_oracle on the same stream (cp_streams.expected, cp_streams.same): status and d are
EQUAL, P is bit for bit, cfo is within 4.2e-12 rad * fs / (2 pi N) (the 1e-8 Hz of
test_cp_search_vs_reference_golden at fs = 30.72 MHz, N = 2048, as an angle), -0.0 where the oracle gives it.
For the non-finite family P is compared by NaN-ness and by value elsewhere.  Each case is one launch with
all streams of a family, as complex128, complex64 and int16.
"""
import math

import numpy as np
import pytest
import torch

import cp_streams as S
import ofdm_oracle as O
from ofdm_sync_amd import _lib, core

pytestmark = pytest.mark.gpu

FMTS = ("c128", "c64", "int16")


def to_device(x, fmt):
    x = np.asarray(x)
    if fmt == "int16":
        return torch.from_numpy(np.stack([x.real, x.imag], -1).astype(np.int16)).cuda()
    return torch.from_numpy(x.astype(np.complex64 if fmt == "c64" else np.complex128)).cuda()


def launch(case, fmt, rows=None):
    """One call of the batched entry point; (status, d, P, cfo) of every stream, on the host."""
    rows = np.arange(len(case.names)) if rows is None else np.asarray(rows)
    xd, est = to_device(case.x[rows], fmt), np.array(case.est[rows])
    if case.op == "cfo":
        cfo, P = core.estimate_cfo_from_cp_batched(xd, est, case.N, case.w, S.FS, return_P=True)
        cfo, P = cfo.cpu().numpy(), P.cpu().numpy()
        return [(0, int(est[k]), P[k], cfo[k]) for k in range(len(rows))]
    cfo, d, P, st = (t.cpu().numpy() for t in core.cp_search_batched(xd, est, case.N, case.w, case.span, case.mode, S.FS))
    return [(st[k], d[k], P[k], cfo[k]) for k in range(len(rows))]


def formats(case):
    return FMTS if S.is_finite(case) else FMTS[:2]           # int16 holds no NaN


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("cfg", S.CONFIGS + ("cfo",), ids=str)
def test_batched_entry_points_equal_the_oracle(cfg, fmt):
    """Every family and stream of one configuration through cp_search_batched / estimate_cfo_from_cp_batched."""
    ran = 0
    for j, case in enumerate(S.cases()):
        if ("cfo" if case.op == "cfo" else (case.N, case.w, case.nb)) != cfg or fmt not in formats(case):
            continue
        got, exp = launch(case, fmt), S.expected(j)
        assert len(got) == len(exp) == len(case.names)
        for b, name in enumerate(case.names):
            assert S.same(got[b], exp[b], case.N, exact=S.is_finite(case)), (
                case.op, case.family, case.mode, cfg, case.span, fmt, name, got[b], exp[b])
        ran += len(got)
    print(f"{cfg} {fmt}: {ran} streams")
    assert ran > 0


def test_all_nan_range_keeps_the_first_offset():
    """The defect this file was written for: a peak search whose every window is NaN reported
    d = INT64_MAX.  One NaN sample with the default span, through the batched call and the drop-ins."""
    seen = 0
    for j, case in enumerate(S.cases()):
        if case.family != "nonfinite" or case.mode != S.PEAK:
            continue
        for b, name in enumerate(case.names):
            st, d, P, cfo = S.expected(j)[b]
            if not (P == 0 and name.startswith("nan_")):
                continue
            lo = max(0, int(case.est[b]) - case.span)
            assert (st, d) == (0, lo) and math.copysign(1.0, cfo) < 0
            got = launch(case, "c64", [b])[0]
            assert (got[0], got[1]) == (0, lo), (case.N, case.w, case.span, name, got)
            assert got[2] == 0 and got[3] == 0 and math.copysign(1.0, got[3]) < 0
            x, e = np.array(case.x[b]), int(case.est[b])
            assert core.find_cp_start_via_corr(x, e, case.N, case.w, search_half=case.span) == lo
            if case.span == case.w // 2:                     # the default span
                c, dd = core.estimate_cfo_from_cp_peak_with_index(x, e, case.N, case.w, S.FS)
                assert dd == lo and c == 0 and math.copysign(1.0, c) < 0
            seen += 1
    assert seen >= 2 * len(S.CONFIGS)


def _fallback_defined(case, b):
    e = int(case.est[b])
    return e >= case.T or (e >= 0 and e + case.N + 2 * case.w <= case.T)


def test_drop_in_functions_equal_the_oracle():
    """The single-stream drop-ins on one stream of every search case (a different one from case to case) and
    on every empty range whose fallback the reference defines, with explicit and default span / win_len."""
    calls = fallbacks = 0
    for j, case in enumerate(S.cases()):
        if case.op != "search" or len(case.names) > 100:
            continue
        exp = S.expected(j)
        pick = {j % len(case.names)} | {b for b in range(len(case.names)) if exp[b][0] == 1}
        for b in sorted(pick):
            if exp[b][0] == 1 and not _fallback_defined(case, b):
                continue
            fallbacks += exp[b][0] == 1
            x, e, N, w = np.array(case.x[b]), int(case.est[b]), case.N, case.w
            if case.nb == 1 and j % 2:
                x = x[0]                                     # 1-D: a single branch
            tag = (case.family, case.mode, N, w, case.nb, case.span, case.names[b])
            dflt = _fallback_defined(case, b)                # a default span may leave the range empty
            with np.errstate(all="ignore"):
                if case.mode == S.PEAK:
                    for span in (case.span, None) if dflt else (case.span,):
                        ec, ed = O.cp_cfo_peak(x, e, N, w, S.FS, span=span)
                        gc, gd = core.estimate_cfo_from_cp_peak_with_index(x, e, N, w, S.FS, span=span)
                        assert gd == ed and S.cfo_same(gc, ec, N), tag + (span, gc, gd, ec, ed)
                        assert S.cfo_same(core.estimate_cfo_from_cp_peak(x, e, N, w, S.FS, span=span), ec, N), tag
                    assert core.find_cp_start_via_corr(x, e, N, w, search_half=case.span) == \
                        O.find_cp_start(x, e, N, w, case.span), tag
                    calls += 3 + 2 * dflt
                else:
                    for kw in (dict(span=case.span, win_len=w), dict(span=case.span), dict(), dict(win_len=w))[:4 if dflt else 2]:
                        ec = O.cp_cfo_robust(x, e, N, 2 * w, S.FS, **kw)
                        gc = core.estimate_cfo_from_cp_robust(x, e, N, 2 * w, S.FS, **kw)
                        assert S.cfo_same(gc, ec, N), tag + (kw, gc, ec)
                    calls += 4 if dflt else 2
    print(f"{calls} drop-in calls, {fallbacks} empty-range fallbacks")
    assert calls > 300 and fallbacks >= 20


def _raw_search(case, fmt, want_P, want_d):
    batch = _lib.as_batch(to_device(case.x, fmt), batched=True)
    dev, B = batch.data.device, batch.B
    est = torch.from_numpy(np.array(case.est)).to(dev)
    cfo = torch.empty((B,), dtype=torch.float64, device=dev)
    st = torch.full((B,), -7, dtype=torch.int32, device=dev)
    P = torch.empty((B, 2), dtype=torch.float64, device=dev) if want_P else None
    d = torch.empty((B,), dtype=torch.int64, device=dev) if want_d else None
    rc = _lib.lib().ofs_cp_search(batch.fmt, batch.data.data_ptr(), B, batch.nb, batch.T, est.data_ptr(), case.N,
                                  case.w, case.span, case.mode, S.FS, P.data_ptr() if want_P else None,
                                  d.data_ptr() if want_d else None, cfo.data_ptr(), st.data_ptr(), _lib.stream_ptr())
    _lib.check(rc, "ofs_cp_search")
    torch.cuda.synchronize()
    return cfo.cpu().numpy(), st.cpu().numpy(), None if P is None else P.cpu().numpy(), None if d is None else d.cpu().numpy()


def test_nullable_outputs():
    """ofs_cp_search with P_out, d_out or both NULL, and ofs_cp_cfo with P_out NULL: cfo and status unchanged
    (bit for bit) on tie, empty-range and non-finite launches of both modes."""
    ran = 0
    for j, case in enumerate(S.cases()):
        if (case.N, case.w, case.nb) != (16, 3, 2) or case.family not in ("ties", "zsum", "empty", "nonfinite"):
            continue
        cfo0, st0, P0, d0 = _raw_search(case, "c64", True, True)
        exp = S.expected(j)
        for b in range(len(case.names)):
            assert S.same((st0[b], d0[b], complex(*P0[b]), cfo0[b]), exp[b], case.N, exact=S.is_finite(case))
        for want_P, want_d in ((False, True), (True, False), (False, False)):
            cfo, st, P, d = _raw_search(case, "c64", want_P, want_d)
            assert np.array_equal(cfo.view(np.int64), cfo0.view(np.int64)) and np.array_equal(st, st0), (case.family, want_P, want_d)
            assert P is None or np.array_equal(P.view(np.int64), P0.view(np.int64))
            assert d is None or np.array_equal(d, d0)
        ran += 1
    assert ran >= 8
    for j, case in enumerate(S.cases()):
        if case.op != "cfo" or case.nb != 2:
            continue
        batch = _lib.as_batch(to_device(case.x, "int16"), batched=True)
        est = torch.from_numpy(np.array(case.est)).cuda()
        cfo = torch.empty((batch.B,), dtype=torch.float64, device="cuda")
        rc = _lib.lib().ofs_cp_cfo(batch.fmt, batch.data.data_ptr(), batch.B, batch.nb, batch.T, est.data_ptr(),
                                   case.N, case.w, S.FS, None, cfo.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "ofs_cp_cfo")
        exp = S.expected(j)
        for b, c in enumerate(cfo.cpu().numpy()):
            assert S.cfo_same(c, exp[b][3], case.N), (case.w, case.names[b])


def test_position_independence():
    """A stream's answer does not depend on its row or on the batch: the tie and non-finite launches of one
    configuration reversed and cut to 1 and 3 streams."""
    for j, case in enumerate(S.cases()):
        if (case.N, case.w, case.nb) != (8, 8, 3) or case.family not in ("ties", "axis", "nonfinite"):
            continue
        B, exp = len(case.names), S.expected(j)
        for order in (list(range(B))[::-1], [B - 1], [2, 0, 1]):
            got = launch(case, "c128", order)
            for k, b in enumerate(order):
                assert S.same(got[k], exp[b], case.N, exact=S.is_finite(case)), (case.family, case.mode, case.names[b], order[:4])
