"""Resumable chunked Park metric with a running peak (csrc/park_chunk.hip, park.ParkChunkedMetric,
ofs_park_metric_chunk).

The yardstick of every case is ONE one-shot batched call on the whole stream (ofs_park_metric, the same
format and precision).  Any chunking must reproduce it BIT FOR BIT: each output concatenated over the
calls, its first 2 * half - 1 elements (d < half, all-zero bits) dropped, begins with the [T - 2 * half]
array of the one-shot call.  One element follows: the output d = T - half, whose window ends at the
stream's last sample; the reference and the one-shot call stop one output earlier, so that element is
checked against a one-shot call on a longer stream (test_newest_output_is_that_of_a_longer_stream).
Every comparison is ``torch.equal`` on integer bit views (a NaN equals the same
NaN, +0.0 differs from -0.0): no tolerance anywhere.  The one thing left out, in
test_non_finite_samples alone, is the sign bit of a word that is NaN in the one-shot result.  The running
peak is checked against ofs_row_argmax on the one-shot M, truncated to the outputs seen so far.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np
import pytest

import park_streams as PS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ofdm_sync_amd import _lib, park  # noqa: E402

KEYS = ("M", "P", "E")
DTYPES = {"c64": torch.complex64, "c128": torch.complex128, "i16": torch.int16}
CD = 2048                                    # outputs of one workgroup tile (csrc/park_tile.h)


# ------------------------------------------------------------------------------------------
# inputs, the one-shot yardstick, comparison
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stream(fmt, nb, B, T, seed=0):
    """[B, nb, T] complex64 / complex128 or [B, nb, T, 2] int16 on the GPU, from a seeded host generator;
    the last stream has a 60 dB loud -> quiet step in its middle.  Computed once per shape, left unchanged."""
    rng = np.random.default_rng(1000 * T + 10 * nb + B + 7919 * seed)
    if fmt == "i16":
        x = rng.integers(-2000, 2001, (B, nb, T, 2))
        x[B - 1, :, T // 2:] = rng.integers(-2, 3, (nb, T - T // 2, 2))
        return torch.from_numpy(x.astype(np.int16)).cuda()
    x = (rng.standard_normal((B, nb, T)) + 1j * rng.standard_normal((B, nb, T))) / np.sqrt(2.0)
    x[B - 1, :, T // 2:] *= 1e-3
    return torch.from_numpy(x.astype(np.complex64 if fmt == "c64" else np.complex128)).cuda()


def _one_shot(x, N):
    ds, M, P, E = park.park_streaming_metric_batched(x, N)
    real = torch.float32 if x.dtype == torch.complex64 else torch.float64
    assert M.dtype == real and E.dtype == real and M.shape == (x.shape[0], x.shape[2] - 2 * (N // 2))
    return {"M": M, "P": P, "E": E}


@functools.lru_cache(maxsize=None)
def _ref(fmt, N, nb, B, T, seed=0):
    """The one-shot call on the whole cached stream (computed once per input, left unchanged)."""
    return _one_shot(_stream(fmt, nb, B, T, seed), N)


def _bits(t):
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _sign(t):
    return 0x7fffffff if t.dtype == torch.int32 else 0x7fffffffffffffff


def _snap(r):
    """Clone of a push result, enqueued on the same stream (the object reuses its buffers)."""
    return park.ParkChunkResult(*[None if t is None else t.clone()
                                  for t in (r.M, r.P, r.E, r.d0, r.peak_index, r.peak_value)])


def _cut(xt, chunks):
    out, s = [], 0
    for c in chunks:
        out.append(xt[:, :, s:s + c].contiguous())
        s += c
    assert s == xt.shape[2], (s, xt.shape)
    return out


def _feed(det, pieces, final=True, flush=False):
    """Push the pieces back to back without any host synchronisation."""
    res = [_snap(det.push(p, final=final and not flush and i == len(pieces) - 1)) for i, p in enumerate(pieces)]
    if flush:
        f = _snap(det.flush())
        assert f.M is None and f.P is None and f.E is None
        res.append(f)
    return res


def _assert_equal(res, ref, N, rows=None, what="", keys=KEYS, nan_sign_free=False):
    """Concatenated outputs: all-zero bits for d < half, then the one-shot arrays bit for bit, then the
    one output d = T - half that the one-shot call does not have.
    nan_sign_free (test_non_finite_samples only): a word that is NaN in the one-shot result is compared
    without its sign bit."""
    fill = 2 * (N // 2) - 1
    body = [r for r in res if any(getattr(r, k) is not None for k in KEYS)]
    for k in keys:
        got = _bits(torch.cat([getattr(r, k) for r in body], dim=1))
        want = _bits(ref[k])
        sel = list(range(want.shape[0])) if rows is None else list(rows)
        assert got.shape[1] == want.shape[1] + fill + 1, (what, k, got.shape, want.shape)
        assert not bool(got[sel][:, :fill].any()), (what, k, "fill phase is not +0.0")
        got = got[:, fill:fill + want.shape[1]]
        if nan_sign_free:
            w = ref[k]
            nan = torch.isnan(torch.view_as_real(w) if w.is_complex() else w)
            got = torch.where(nan, got & _sign(got), got)
            want = torch.where(nan, want & _sign(want), want)
        if not torch.equal(got[sel], want[sel]):
            bad = (got[sel] != want[sel]).nonzero()
            raise AssertionError((what, k, "first differing [row, index(, part)]", bad[0].tolist(), "of", len(bad)))


def _assert_d0(res, chunks, N, what=""):
    """d0 of call i = (samples of earlier calls) - half + 1, for every stream."""
    seen = 0
    for r, c in zip(res, list(chunks) + [0]):
        assert r.d0.tolist() == [seen - N // 2 + 1] * r.d0.shape[0], (what, seen, r.d0.tolist())
        seen += c


def _row_argmax(M):
    """ofs_row_argmax on M [B, n], n >= 1: (index [B] int64, value [B] float64)."""
    B, n = M.shape
    M = M.contiguous()
    idx = torch.empty((B,), dtype=torch.int64, device=M.device)
    val = torch.empty((B,), dtype=torch.float64, device=M.device)
    prec = _lib.FP32 if M.dtype == torch.float32 else _lib.FP64
    _lib.check(_lib.lib().ofs_row_argmax(prec, M.data_ptr(), B, n, idx.data_ptr(), val.data_ptr(), _lib.stream_ptr()),
               "ofs_row_argmax")
    return idx, val


def _assert_peak(r, Mref, seen, N, rows=None, what=""):
    """After a call that brought the stream to `seen` samples: the peak is ofs_row_argmax of the one-shot
    M truncated to the seen - 2 * half valid outputs (index + half), or (-1, 0.0) without any."""
    half = N // 2
    nv = min(seen - 2 * half, Mref.shape[1])
    sel = list(range(Mref.shape[0])) if rows is None else list(rows)
    if nv <= 0:
        assert r.peak_index[sel].tolist() == [-1] * len(sel) and r.peak_value[sel].tolist() == [0.0] * len(sel), \
            (what, seen, r.peak_index.tolist(), r.peak_value.tolist())
        return
    idx, val = _row_argmax(Mref[:, :nv])
    assert torch.equal(r.peak_index[sel], idx[sel] + half), (what, seen, r.peak_index.tolist(), (idx + half).tolist())
    a, b = r.peak_value[sel], val[sel]
    assert bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()), (what, seen, a.tolist(), b.tolist())


def _assert_peaks(res, chunks, Mref, N, rows=None, what=""):
    seen = 0
    for r, c in zip(res, list(chunks) + [0]):
        seen += c
        _assert_peak(r, Mref, seen, N, rows=rows, what=what)


def _rest(T, head):
    head = [int(c) for c in head]
    assert sum(head) < T, (T, head)
    return head + [T - sum(head)]


def _even(T, c):
    n = (T - 1) // c
    return [c] * n + [T - c * n]


def _random_split(rng, T, top):
    out = []
    while sum(out) < T:
        out.append(min(int(rng.integers(1, top + 1)), T - sum(out)))
    return out


def _odd_split(rng, T, top):
    """All sizes odd (never a multiple of 8)."""
    out = []
    while T - sum(out) > top:
        out.append(2 * int(rng.integers(0, top // 2)) + 1)
    r = T - sum(out)
    out += [r] if r % 2 else [1, r - 1]
    assert sum(out) == T and all(c % 2 for c in out)
    return out


def _chunkings(N, T, seed):
    """The whole stream; equal chunks of 1024; a seeded random split (pieces up to 2N); all-odd sizes;
    chunks shorter than the history, one sample at a time over the first 40 samples and across
    n = 2 * half - 1; exactly 2 * half - 1 samples, then 1; a boundary on the edge of the first 2048-output
    tile and one sample to each side of it (where the stream is that long)."""
    half = N // 2
    fill = 2 * half - 1
    rng = np.random.default_rng(seed)
    out = [[T], _even(T, 1024), _random_split(rng, T, 2 * N), _odd_split(rng, T, max(2 * N, 16))]
    short = [1] * 40
    while sum(short) < fill - 3:
        short.append(min(int(rng.integers(1, 2 * half)), fill - 3 - sum(short)))
    short += [1] * 6                                            # n = fill - 3 .. fill + 2, one at a time
    while T - sum(short) > 2 * half:
        short.append(int(rng.integers(1, 2 * half)))
    out.append(_rest(T, short))
    out.append(_rest(T, [fill, 1]))
    edge = CD + fill                                            # samples before output i = 2048
    if T > edge + 1:
        out += [_rest(T, [edge]), _rest(T, [edge - 1]), _rest(T, [edge + 1]), _rest(T, [half, edge - half, 1])]
    return out


def _detector(fmt, B, nb, N, **kw):
    return park.ParkChunkedMetric(B, nb, N, dtype=DTYPES[fmt], **kw)


# ------------------------------------------------------------------------------------------
# 1. any chunking equals the one-shot call
# ------------------------------------------------------------------------------------------
SHAPES = [(8, 1, 3, 300), (30, 1, 3, 700), (64, 2, 3, 5000), (256, 1, 3, 3000), (256, 2, 3, 3000),
          (2048, 1, 2, 7000)]
CASES = [(N, nb, B, T, fmt) for (N, nb, B, T) in SHAPES for fmt in ("c64", "c128", "i16")
         if N != 2048 or fmt == "c64"]


@pytest.mark.parametrize("N,nb,B,T,fmt", CASES)
def test_any_chunking_equals_one_shot(N, nb, B, T, fmt):
    """N = 8: half < 7, the per-output energy; 30: odd half; 64 x 2 branches: three 2048-output tiles;
    256; 2048: the history is read by two tiles.  The same object throughout: each final call (or flush)
    leaves fresh streams for the next chunking.  d0 of every call and the last peak are checked too."""
    ref = _ref(fmt, N, nb, B, T)
    xt = _stream(fmt, nb, B, T)
    det = _detector(fmt, B, nb, N)
    assert det.max_chunk == 1 << 30
    runs = []
    for i, chunks in enumerate(_chunkings(N, T, seed=N + nb)):
        assert sum(chunks) == T and min(chunks) >= 1
        runs.append((chunks, _feed(det, _cut(xt, chunks), final=True, flush=(i % 2 == 1))))
        assert det.samples_seen == 0
    torch.cuda.synchronize()
    for chunks, res in runs:
        what = f"{fmt} N={N} nb={nb} chunks {chunks[:6]}... ({len(chunks)})"
        _assert_equal(res, ref, N, what=what)
        _assert_d0(res, chunks, N, what=what)
        _assert_peak(res[-1], ref["M"], T, N, what=what)


@pytest.mark.parametrize("N,nb,B,T,fmt", [(8, 1, 3, 300, "c64"), (64, 2, 3, 5000, "i16"), (256, 1, 3, 3000, "c128")])
def test_newest_output_is_that_of_a_longer_stream(N, nb, B, T, fmt):
    """After T - 40 samples the newest element (d = T - 40 - half) is what the one-shot call returns at
    that d on the whole stream, and it is not in the peak until the next sample arrives."""
    ref = _ref(fmt, N, nb, B, T)
    xt = _stream(fmt, nb, B, T)
    S = T - 40
    det = _detector(fmt, B, nb, N)
    chunks = [S - 1, 1, 1]
    res = _feed(det, _cut(xt[:, :, :S + 1].contiguous(), chunks))
    torch.cuda.synchronize()
    for k in KEYS:
        got = _bits(torch.cat([getattr(r, k) for r in res], dim=1))[:, N // 2 * 2 - 1:]
        assert torch.equal(got, _bits(ref[k][:, :got.shape[1]])) and got.shape[1] == S + 1 - 2 * (N // 2) + 1, k
    _assert_peaks(res, chunks, ref["M"], N, what="newest output")


# ------------------------------------------------------------------------------------------
# 2. the running peak
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nb,B,T,fmt", [(30, 1, 3, 700, "c64"), (64, 2, 3, 5000, "i16"), (256, 1, 3, 3000, "c128"),
                                          (2048, 1, 2, 7000, "c64")])
def test_running_peak_on_random_streams(N, nb, B, T, fmt):
    """After every push: ofs_row_argmax of the one-shot M truncated to the outputs seen so far."""
    ref = _ref(fmt, N, nb, B, T)
    xt = _stream(fmt, nb, B, T)
    det = _detector(fmt, B, nb, N, outputs=("M",))
    rng = np.random.default_rng(N)
    runs = [(c, _feed(det, _cut(xt, c), flush=f)) for c, f in ((_random_split(rng, T, N), False),
                                                               (_random_split(rng, T, 3 * N), True))]
    torch.cuda.synchronize()
    for chunks, res in runs:
        _assert_peaks(res, chunks, ref["M"], N, what=f"{fmt} N={N} {chunks[:6]}")


def test_running_peak_on_the_tie_stream():
    """Three exactly tied maxima (M = 1.0) in three different pushes, behind a smaller local maximum
    (tests/test_park_streams_host.py): the first tie replaces it and the later ties do not replace the first."""
    N = PS.TIE_N
    x = torch.from_numpy(PS.tie_stream()).cuda()
    ref = _one_shot(x, N)
    for chunks in (list(PS.TIE_CHUNKS), [PS.TIE_T], _even(PS.TIE_T, 7)):
        det = _detector("i16", 2, 1, N)
        res = _feed(det, _cut(x, chunks))
        torch.cuda.synchronize()
        _assert_equal(res, ref, N, what="tie stream")
        _assert_peaks(res, chunks, ref["M"], N, what=f"tie stream {chunks[:5]}")
        assert res[-1].peak_index.tolist() == [PS.tie_centres(0)[0], PS.tie_centres(1)[0]]
        assert res[-1].peak_value.tolist() == [1.0, 1.0]
    # the pushes of TIE_CHUNKS, one by one: the peak before the first centre's push is another, smaller one
    det = _detector("i16", 2, 1, N)
    res = _feed(det, _cut(x, list(PS.TIE_CHUNKS)))
    first = PS.call_of_d(PS.TIE_CHUNKS, PS.tie_centres(0)[0], N)
    assert 0.0 < float(res[first - 1].peak_value[0]) < 1.0 and float(res[first].peak_value[0]) == 1.0


def test_running_peak_on_the_nan_stream():
    """The first NaN of M wins from its push on, although a larger number follows in a later push; the
    stream without the NaN peaks at that number."""
    N = PS.NAN_N
    x = torch.from_numpy(PS.nan_stream()).cuda()
    ref = _one_shot(x, N)
    for chunks in (list(PS.NAN_CHUNKS), [PS.NAN_T], _even(PS.NAN_T, 33)):
        det = _detector("c64", 2, 1, N)
        res = _feed(det, _cut(x, chunks), flush=True)
        torch.cuda.synchronize()
        _assert_peaks(res, chunks, ref["M"], N, what=f"nan stream {chunks[:5]}")
        assert res[-1].peak_index.tolist() == [PS.nan_first_d(), PS.NAN_BLOCK + N // 2 - 1]
        assert bool(torch.isnan(res[-1].peak_value[0])) and abs(float(res[-1].peak_value[1]) - 1.0) < 1e-5
    det = _detector("c64", 2, 1, N)
    res = _feed(det, _cut(x, list(PS.NAN_CHUNKS)))
    c = PS.call_of_d(PS.NAN_CHUNKS, PS.nan_first_d(), N)
    assert not bool(torch.isnan(res[c - 1].peak_value[0])) and bool(torch.isnan(res[c].peak_value[0]))


def test_peak_needs_M():
    """Without an M the peak does not move (a flush reports no peak although outputs were produced), and
    asking for it in a call without M is refused."""
    N, nb, B, T = 64, 2, 3, 5000
    xt = _stream("c64", nb, B, T)
    det = _detector("c64", B, nb, N, outputs=("P", "E"), track_peak=False)
    r = det.push(xt[:, :, :1000].contiguous())
    assert r.M is None and r.peak_index is None and r.peak_value is None and r.P is not None
    pi = torch.full((B,), 77, dtype=torch.int64, device="cuda")
    pv = torch.full((B,), 77.0, dtype=torch.float64, device="cuda")
    x2 = xt[:, :, 1000:1100].contiguous()
    args = (B, nb, 100, N, _lib.FP32, det.state.data_ptr(), None, r.P.data_ptr(), None, None)
    rc = det._fn(_lib.C64, x2.data_ptr(), *args, pi.data_ptr(), None, 0, _lib.stream_ptr())
    with pytest.raises(ValueError):
        _lib.check(rc, "ofs_park_metric_chunk")
    rc = det._fn(_lib.C64, x2.data_ptr(), *args, None, pv.data_ptr(), 0, _lib.stream_ptr())
    with pytest.raises(ValueError):
        _lib.check(rc, "ofs_park_metric_chunk")
    d0 = torch.zeros((B,), dtype=torch.int64, device="cuda")
    rc = det._fn(_lib.C64, None, B, nb, 0, N, _lib.FP32, det.state.data_ptr(), None, None, None, d0.data_ptr(),
                 pi.data_ptr(), pv.data_ptr(), 1, _lib.stream_ptr())            # the flush, with peak outputs
    _lib.check(rc, "ofs_park_metric_chunk")
    assert d0.tolist() == [1000 - N // 2 + 1] * B                               # the refused calls changed nothing
    assert pi.tolist() == [-1] * B and pv.tolist() == [0.0] * B
    # track_peak=True without "M" in outputs: the peak is there, M is not returned
    ref = _ref("c64", N, nb, B, T)
    det = _detector("c64", B, nb, N, outputs=("E",))
    res = _feed(det, _cut(xt, _rest(T, [1000, 100])))
    assert all(q.M is None and q.P is None for q in res)
    _assert_equal(res, ref, N, keys=("E",))
    _assert_peaks(res, _rest(T, [1000, 100]), ref["M"], N)


# ------------------------------------------------------------------------------------------
# 3. outputs
# ------------------------------------------------------------------------------------------
def test_requested_outputs():
    """Every subset of M / P / E is bitwise that of the full call; with outputs=() and no peak nothing is
    stored and the state still advances."""
    N, nb, B, T = 256, 1, 3, 3000
    ref = _ref("c64", N, nb, B, T)
    xt = _stream("c64", nb, B, T)
    chunks = _rest(T, [N + 11, 1, 300, 255])
    pieces = _cut(xt, chunks)
    runs = []
    for n in range(4):
        for want in itertools.combinations(KEYS, n):
            det = _detector("c64", B, nb, N, outputs=want, track_peak=n % 2 == 0)
            res = _feed(det, pieces)
            assert all(getattr(r, k) is None for r in res for k in KEYS if k not in want)
            assert all((r.peak_index is None) == (n % 2 == 1) for r in res)
            runs.append((want, res))
    none = _detector("c64", B, nb, N, outputs=(), track_peak=False)
    quiet = _feed(none, pieces[:3], final=False)
    assert none.samples_seen == sum(chunks[:3])
    tail = _detector("c64", B, nb, N)
    tail.state.copy_(none.state)                                 # a storing object takes the state over
    rest = _feed(tail, pieces[3:])
    torch.cuda.synchronize()
    for want, res in runs:
        _assert_equal(res, ref, N, keys=want, what=f"outputs {want}")
        _assert_d0(res, chunks, N, what=f"outputs {want}")
        if res[-1].peak_index is not None:
            _assert_peaks(res, chunks, ref["M"], N, what=f"outputs {want}")
    _assert_d0(quiet, chunks[:3], N, what="outputs ()")
    s = sum(chunks[:3])
    for k in KEYS:
        got = torch.cat([getattr(r, k) for r in rest], dim=1)[:, :-1]
        assert torch.equal(_bits(got), _bits(ref[k][:, s - (N - 1):])), k


# ------------------------------------------------------------------------------------------
# 4. fill phase and d0
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["c64", "c128"])
def test_fill_phase_is_zero_over_nan_buffers(fmt):
    """d < half: all-zero bits, written over result buffers pre-filled with NaN, also when the first
    samples are NaN or Inf, whatever the chunking; d0 on every call; no peak before the first output."""
    N, nb, B, T = 64, 1, 4, 400
    fill = N - 1
    x = _stream(fmt, nb, B, T).clone()
    x[0, 0, 0] = float("nan")
    x[1, 0, 5] = complex(float("inf"), 0.0)
    x[2, 0, fill - 1] = complex(0.0, float("nan"))
    ref = _one_shot(x, N)
    det = _detector(fmt, B, nb, N)
    splits = ([T], _rest(T, [3] * (fill // 3 + 2)), _rest(T, [fill - 1, 1, 1, 1]), _rest(T, [1, N // 2, N // 2 + 1]))
    runs = []
    for c in splits:
        for Tc in set(c):
            r = det._buffers(Tc)[0]                               # the buffers the pushes of Tc samples write
            r.M.fill_(float("nan"))
            r.E.fill_(float("nan"))
            r.P.fill_(complex(float("nan"), float("nan")))
        runs.append((c, _feed(det, _cut(x, c), flush=True)))
    torch.cuda.synchronize()
    for chunks, res in runs:
        _assert_d0(res, chunks, N, what=f"fill {chunks[:5]}")
        for k in KEYS:
            head = torch.cat([getattr(r, k) for r in res[:-1]], dim=1)[:, :fill]
            assert head.shape[1] == fill and not bool(_bits(head).any()), (k, chunks[:5])
        _assert_equal(res, ref, N, rows=(3,), what=f"fill {chunks[:5]}")
        _assert_equal(res, ref, N, what=f"fill {chunks[:5]}", nan_sign_free=True)
        seen = 0
        for r, c in zip(res, chunks):
            seen += c
            if seen < 2 * (N // 2) + 1:
                assert r.peak_index.tolist() == [-1] * B and r.peak_value.tolist() == [0.0] * B


# ------------------------------------------------------------------------------------------
# 5. partial reset: streams at different n in one launch
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nb,fmt", [(30, 1, "c64"), (256, 2, "i16"), (256, 1, "c128")])
def test_partial_reset(N, nb, fmt):
    """reset(mask) / a memset of state rows after two chunks: the reset streams continue as a one-shot
    call on the remaining samples (their own fill phase, their own peak), the others are unaffected."""
    B, T = 6, 3000 if N == 256 else 700
    half = N // 2
    s = N + 2 * half // 3 + 5
    chunks = [s - 7, 7] + _rest(T - s, [N - 3, 5, half + 1])
    x = _stream(fmt, nb, B, T)
    ref = _ref(fmt, N, nb, B, T)
    tail = _one_shot(x[:, :, s:].contiguous(), N)
    pieces = _cut(x, chunks)
    det = _detector(fmt, B, nb, N)
    res = _feed(det, pieces[:2], final=False)
    det.reset(torch.tensor([True, False, False, True, False, False]))
    det.state[4].zero_()                                               # the documented memset of a state row
    res += _feed(det, pieces[2:], final=True)
    torch.cuda.synchronize()
    _assert_equal(res, ref, N, rows=(1, 2, 5), what="kept")
    _assert_equal(res[2:], tail, N, rows=(0, 3, 4), what="reset")
    _assert_peaks(res, chunks, ref["M"], N, rows=(1, 2, 5), what="kept")
    _assert_peaks(res[2:], chunks[2:], tail["M"], N, rows=(0, 3, 4), what="reset")
    assert res[2].d0.tolist() == [-half + 1 if b in (0, 3, 4) else s - half + 1 for b in range(B)]
    assert res[3].d0.tolist() == [chunks[2] - half + 1 + (0 if b in (0, 3, 4) else s) for b in range(B)]
    det.push(pieces[0])
    det.reset()
    assert det.samples_seen == 0 and not bool(det.state.any())


# ------------------------------------------------------------------------------------------
# 6. final, flush, shortest streams
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["c64", "i16"])
def test_final_and_flush_leave_fresh_streams(fmt):
    """A stream abandoned in the middle by push(final=True) or flush(): the next push starts a fresh
    stream (its peak too); final changes no output of its own call."""
    N, nb, B, T = 256, 1, 3, 3000
    ref = _ref(fmt, N, nb, B, T)
    xt = _stream(fmt, nb, B, T)
    cut = N + 2 * 128 + 17
    head = _one_shot(xt[:, :, :cut].contiguous(), N)
    det = _detector(fmt, B, nb, N)
    pieces = _cut(xt, _rest(T, [300, cut - 300]))
    a = _feed(det, pieces[:2], final=True)                             # ends after `cut` samples
    assert det.samples_seen == 0
    ch_b = _rest(T, [N, 333])
    b = _feed(det, _cut(xt, ch_b), final=False)                        # a fresh stream: the whole input
    assert det.samples_seen == T
    f = _snap(det.flush())
    c = _feed(det, pieces, final=False)
    det.flush()
    d = _feed(det, [xt], final=True)
    torch.cuda.synchronize()
    _assert_equal(a, head, N, what="ended by final")
    _assert_peaks(a, [pieces[0].shape[2], pieces[1].shape[2]], head["M"], N, what="ended by final")
    _assert_equal(b, ref, N, what="after final")
    _assert_peaks(b, ch_b, ref["M"], N, what="after final")
    assert f.d0.tolist() == [T - N // 2 + 1] * B
    _assert_peak(f, ref["M"], T, N, what="flush")
    _assert_equal(c, ref, N, what="after flush")
    _assert_equal(d, ref, N, what="after flush, one push")
    _assert_peak(d[0], ref["M"], T, N, what="after flush, one push")


@pytest.mark.parametrize("N,fmt", [(8, "c64"), (30, "c128"), (256, "i16"), (2048, "c64")])
def test_shortest_streams(N, fmt):
    """Exactly 2 * half + 1 samples: one output of the one-shot call, whole or as 2 * half samples and 1.
    One sample less: the reference has no output and the peak stays -1; the one element behind the fill
    phase (d = half, its window is complete) is that one output of the longer stream."""
    half, B = N // 2, 3
    T = 2 * half + 1
    x = _stream(fmt, 1, B, 2 * half + 40)[:, :, :T].contiguous()
    ref = _one_shot(x, N)
    assert ref["M"].shape == (B, 1)
    det = _detector(fmt, B, 1, N)
    runs = [(c, _feed(det, _cut(x, c), flush=fl)) for c, fl in (([T], False), ([T - 1, 1], True), ([1, T - 2, 1], False))]
    short = _feed(det, [x[:, :, :T - 1].contiguous()], flush=True)
    torch.cuda.synchronize()
    for chunks, res in runs:
        _assert_equal(res, ref, N, what=f"one output {chunks}")
        _assert_peaks(res, chunks, ref["M"], N, what=f"one output {chunks}")
        assert res[-1].peak_index.tolist() == [half] * B
    for k in KEYS:
        got = _bits(getattr(short[0], k))
        assert getattr(short[0], k).shape == (B, T - 1) and not bool(got[:, :T - 2].any()), k
        assert torch.equal(got[:, T - 2:], _bits(ref[k])), k
    for r in short:
        assert r.peak_index.tolist() == [-1] * B and r.peak_value.tolist() == [0.0] * B
    assert short[1].d0.tolist() == [T - 1 - half + 1] * B


# ------------------------------------------------------------------------------------------
# 7. non-finite samples
# ------------------------------------------------------------------------------------------
def test_non_finite_samples():
    """One NaN, one +Inf and one -Inf sample, each in a stream of its own: bitwise equal where the
    one-shot word is not NaN, a NaN where it is (the sign of a NaN is outside the guarantee: it depends on
    the operand order of an operation on two NaNs, which is the compiler's)."""
    N, nb, B, T = 256, 1, 4, 3000
    x = _stream("c64", nb, B, T).clone()
    x[0, 0, N + 3] = float("nan")
    x[1, 0, N + 3] = complex(float("inf"), 0.0)
    x[2, 0, 2 * N + 100] = complex(1.0, float("-inf"))
    ref = _one_shot(x, N)
    for b in (0, 1):
        assert bool(torch.isnan(torch.view_as_real(ref["P"][b])).any()) and bool(torch.isnan(ref["M"][b]).any()), b
    # 1 - inf j: every product has one infinite factor, P is +-Inf without a NaN; M = Inf / Inf is NaN
    assert bool(torch.isinf(torch.view_as_real(ref["P"][2])).any()) and bool(torch.isnan(ref["M"][2]).any())
    assert bool(torch.isfinite(ref["M"][3]).all()) and bool(torch.isfinite(ref["E"][3]).all())
    det = _detector("c64", B, nb, N)
    rng = np.random.default_rng(5)
    splits = [[T], _rest(T, [N + 3, 1]), _rest(T, [N + 4, 255, 257]), _random_split(rng, T, N), _even(T, 255)]
    runs = [(c, _feed(det, _cut(x, c))) for c in splits]
    torch.cuda.synchronize()
    for chunks, res in runs:
        _assert_equal(res, ref, N, what=f"non-finite {chunks[:5]}", nan_sign_free=True)
        _assert_equal(res, ref, N, rows=(3,), what=f"finite stream {chunks[:5]}")
        _assert_peaks(res, chunks, ref["M"], N, what=f"non-finite {chunks[:5]}")


# ------------------------------------------------------------------------------------------
# 8. the energy variant, limits, bad chunks
# ------------------------------------------------------------------------------------------
def test_park_direct_variant_is_followed(variant):
    """PARK_DIRECT (per-output energy sums) selects the energy form of both calls: the pair stays equal."""
    N, nb, B, T = 64, 2, 3, 5000
    xt = _stream("c64", nb, B, T)
    variant("PARK_DIRECT", 1)
    ref = _one_shot(xt, N)
    chunks = _random_split(np.random.default_rng(2), T, 2 * N)
    res = _feed(_detector("c64", B, nb, N), _cut(xt, chunks))
    torch.cuda.synchronize()
    _assert_equal(res, ref, N, what="PARK_DIRECT")


def test_limits_and_bad_chunks_raise_value_error():
    for N, dt in ((8192, torch.complex64), (8191, torch.complex64), (4096, torch.complex128), (4095, torch.int16),
                  (1, torch.complex64), (0, torch.int16)):
        with pytest.raises(ValueError):
            park.ParkChunkedMetric(2, 1, N, dtype=dt)
    for dt in (torch.float32, torch.float64, torch.int32, torch.uint8, torch.complex32):
        with pytest.raises(ValueError):
            park.ParkChunkedMetric(2, 1, 64, dtype=dt)
    with pytest.raises(ValueError):
        park.ParkChunkedMetric(2, 0, 64)
    with pytest.raises(ValueError):
        park.ParkChunkedMetric(2, 1, 64, outputs=("M", "R"))
    assert park.ParkChunkedMetric(1, 1, 8190).N == 8190 and park.ParkChunkedMetric(1, 2, 4094, dtype=torch.int16).N == 4094
    # unsupported (format, precision) pairs at the ABI
    st = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for f, p in ((_lib.C64, _lib.FP64), (_lib.C128, _lib.FP32), (_lib.CI16, _lib.FP32), (_lib.CP12, _lib.FP64)):
        rc = _lib.lib().ofs_park_metric_chunk(f, st.data_ptr(), 1, 1, 4, 64, p, st.data_ptr(), None, None, None, None,
                                              None, None, 0, _lib.stream_ptr())
        with pytest.raises(ValueError):
            _lib.check(rc, "ofs_park_metric_chunk")
    det = park.ParkChunkedMetric(2, 2, 64)
    assert det.N == 64 and park.ParkChunkedMetric(1).N == park.N_FFT       # N=None reads park.N_FFT
    good = torch.zeros((2, 2, 10), dtype=torch.complex64, device="cuda")
    for bad in (good.to(torch.complex128), good[:1], good[:, :1], good[:, 0], good[:, :, :0], np.zeros((2, 2, 10), np.complex64),
                torch.zeros((2, 2, 10, 2), dtype=torch.int16, device="cuda")):
        with pytest.raises(ValueError):
            det.push(bad)
    assert det.samples_seen == 0 and not bool(det.state.any())
    di = park.ParkChunkedMetric(2, 1, 64, dtype=torch.int16)
    for bad in (torch.zeros((2, 10), dtype=torch.int16, device="cuda"), torch.zeros((2, 10, 3), dtype=torch.int16, device="cuda"),
                good):
        with pytest.raises(ValueError):
            di.push(bad)
    r = di.push(torch.zeros((2, 10, 2), dtype=torch.int16, device="cuda"))      # [B, Tc, 2] for one branch
    assert r.M.shape == (2, 10) and r.M.dtype == torch.float64 and di.samples_seen == 10
