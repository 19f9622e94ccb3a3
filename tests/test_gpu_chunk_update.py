"""The update path the chunked Park and zc_freq metrics share (csrc/chunk_state.h: ring write-back,
row scan, peak fold), on the cases tests/test_gpu_park_chunked.py and tests/test_gpu_zc_freq_chunked.py do
not reach together in one stream: pushes of one sample, pushes shorter than, exactly as long as and longer
than the ring Hr (the ring wraps and is overwritten whole), a maximum tied across a push boundary, and a
NaN that arrives in a later push than the maximum it replaces.

Inputs are exact: a stream of zeros, and small-integer streams (entries of {1, j, -1, -j} from
tests/exact_streams.py, doubled) that repeat with a period that keeps every output's place in its tile /
chunk, so outputs one period apart are equal in every bit.  The yardsticks are those of the two detectors'
own suites, whose helpers do the comparing: ONE one-shot call on the whole stream, bit for bit, and
ofs_row_argmax of its metric truncated to the outputs seen after each push.  The smallest shapes: Park
N = 8 (half = 4, Hr = 24), zc_freq N = 64, cp = 5 (C = 64, Hr = 128), B = 3, a few rings of samples.
"""
from __future__ import annotations

import numpy as np
import pytest

import exact_streams as ES
import park_streams as PS
import test_gpu_park_chunked as TP
import test_gpu_zc_freq_chunked as TZ

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ofdm_sync_amd import _lib  # noqa: E402

B = 3
SAMPLE_BYTES = {"c64": 8, "c128": 16, "i16": 4}


def _streams(nb, T, period, nan_at):
    """complex128 [3, nb, T]: zeros; a stream of period ``period``; another, with a NaN sample at
    ``nan_at`` of its last branch (None: without)."""
    reps = T // period + 1
    x = np.zeros((B, nb, T), np.complex128)
    for r in range(nb):
        x[1, r] = np.tile(2 * ES.unit(period, 11 + r), reps)[:T]
        x[2, r] = np.tile(2 * ES.unit(period, 23 + r), reps)[:T]
    if nan_at is not None:
        x[2, nb - 1, nan_at] = complex(np.nan, 1.0)
    return x


def _chunks(Hr, T):
    """One sample (three times), shorter than the ring, the ring's length, longer, one sample, the ring's
    length again (every slot is overwritten by one call), two rings and more, a short one, the rest."""
    head = [1, 1, 1, Hr // 3, Hr, Hr + 7, 1, Hr, 2 * Hr + 2, 5]
    assert sum(head) < T
    return head + [T - sum(head)]


def _scenario(M, chunks, first_sample_after, nan_row):
    """From the one-shot metric: row 1's maximum is tied and its first and last places join the peak in
    different pushes; row 2 (if it has the NaN) holds a number as its peak in an earlier push than the one
    whose outputs turn NaN.  ``first_sample_after(i)``: the sample that must arrive for output i to count."""
    Mh = M.double().cpu().numpy()
    call = lambda i: PS.call_of_sample(chunks, first_sample_after(i))   # noqa: E731
    top = np.flatnonzero(Mh[1] == np.nanmax(Mh[1]))
    assert top.size >= 2 and call(top[0]) < call(top[-1]), ("no tie across a push boundary", top[:4])
    if nan_row:
        nan = np.flatnonzero(np.isnan(Mh[2]))
        assert nan.size and nan[0] > 0
        best = int(np.argmax(Mh[2, :nan[0]]))
        assert call(best) < call(nan[0]), ("the NaN is not later than the maximum", best, nan[0])


def _assert_row_argmax(M, index, value, offset):
    idx, val = TP._row_argmax(M)
    assert torch.equal(index, idx + offset), (index.tolist(), idx.tolist())
    assert bool(((value == val) | (torch.isnan(value) & torch.isnan(val))).all()), (value.tolist(), val.tolist())


@pytest.mark.parametrize("fmt", ["c64", "i16"])
def test_park_update_path(fmt):
    N, nb, Hr = 8, 1, 24
    half, T = N // 2, 7 * 24 + 2
    assert _lib.lib().ofs_park_chunk_state_bytes(TZ.FMTS[fmt], nb, N) == 64 + nb * Hr * SAMPLE_BYTES[fmt]
    chunks = _chunks(Hr, T)
    nan_at = sum(chunks[:7]) + 3 if fmt == "c64" else None              # in the second push of Hr samples
    x = TZ._to_dev(_streams(nb, T, 8, nan_at), fmt)                     # period 8 = outputs per thread (OPT)
    ref = TP._one_shot(x, N)
    _scenario(ref["M"], chunks, lambda i: i + 2 * half, nan_row=nan_at is not None)
    for flush in (False, True):
        det = TP._detector(fmt, B, nb, N)
        res = TP._feed(det, TP._cut(x, chunks), flush=flush)
        torch.cuda.synchronize()
        TP._assert_equal(res, ref, N, what=f"park {fmt}", nan_sign_free=nan_at is not None)
        TP._assert_d0(res, chunks, N)
        TP._assert_peaks(res, chunks, ref["M"], N, what=f"park {fmt}")  # ofs_row_argmax after every push
        _assert_row_argmax(ref["M"], res[-1].peak_index, res[-1].peak_value, half)
        assert det.samples_seen == 0


@pytest.mark.parametrize("fmt,nb", [("c128", 1), ("c64", 2), ("i16", 2)])
def test_zc_freq_update_path(fmt, nb):
    N, cp, Hr = 64, 5, 128
    need, T = N + cp, 7 * 128 + 4
    assert TZ._C(N) == 64
    assert _lib.lib().ofs_zc_freq_chunk_state_bytes(TZ.FMTS[fmt], nb, N, cp) == 64 + nb * Hr * SAMPLE_BYTES[fmt]
    chunks = _chunks(Hr, T)
    nan_at = sum(chunks[:7]) + 3 if fmt != "i16" else None
    xd = TZ._to_dev(_streams(nb, T, 64, nan_at), fmt)                   # period 64 = the chunk length C
    tmpl = TZ._template()
    ref = TZ._one_shot(xd, N, cp, tmpl)
    _scenario(ref, chunks, lambda i: i + need - 1, nan_row=nan_at is not None)
    det = TZ._det(xd, N, cp)
    res = TZ._feed(det, xd, chunks)
    # the metric bit for bit, off0, and the peak after every push against the first argmax so far
    TZ._check(res, ref, N, cp, what=f"zc_freq {fmt} nb={nb}", nan_sign_free=nan_at is not None)
    _assert_row_argmax(ref, res[-1].pi, res[-1].pv, 0)
    seen = 0
    for r, c in zip(res, chunks):                                        # ofs_row_argmax itself, after every push
        seen += c
        if seen >= need:
            _assert_row_argmax(ref[:, :seen - need + 1], r.pi, r.pv, 0)
    assert det.n_seen == 0
