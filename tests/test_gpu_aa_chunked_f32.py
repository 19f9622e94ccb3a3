"""Resumable chunked [A][A] detection for complex64 streams (csrc/aa_chunk_f32.hip,
sync_aa.AAChunkedDetectorF32, ofs_aa_detect_chunk_f32).

The yardstick of every case is ONE ``ofs_aa_detect(OFS_C64, ..., OFS_FP32)`` call with P, R, M (and
valid) present on the whole stream, on plans 1000-1099 (even T <= 1024, aa_fast_kernel) and 1100-1199
(any other T, aa_stream_kernel).  Any chunking must reproduce it BIT FOR BIT: the concatenated P, R, M,
valid and the sequence of events, integers and reals.  Every comparison is ``torch.equal`` on the bit
patterns (int32 / int64 views, so a NaN equals the same NaN and +0.0 differs from -0.0): no tolerance
anywhere against the one-shot call (the one thing left out, in test_non_finite_head alone and for the
reason given there, is the sign bit of a word that is NaN in the one-shot result).  The fp32 arithmetic is not exact, so this holds only if a call
continues the same fp32 partials, the same fp64 row scans and the same carried fp64 bases.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import exact_streams as X

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ofdm_sync_amd import _lib, sync_aa  # noqa: E402

THR = 0.15
OUT = ("P", "R", "M", "valid")


# ------------------------------------------------------------------------------------------
# inputs, the one-shot yardstick, comparison
# ------------------------------------------------------------------------------------------
def _bursts(seed, B, nb, T, L, noise=0.05):
    """complex64 [B, nb, T]: noise plus two (T < 5L) or three [A][A] bursts per stream, spread over the
    stream and shifted by 3 samples from stream to stream; the last one may be cut off by the end of the
    stream (a gate that is still open at T)."""
    rng = np.random.default_rng(seed)
    x = noise * (rng.standard_normal((B, nb, T)) + 1j * rng.standard_normal((B, nb, T)))
    k = 2 if T < 5 * L else 3
    for b in range(B):
        for i in range(k):
            s = (i * T) // k + 3 * b
            a = (rng.standard_normal(L) + 1j * rng.standard_normal(L)) * np.exp(2j * np.pi * rng.random())
            n = min(2 * L, T - s)
            x[b, :, s:s + n] += np.tile(a, 2)[:n] * (0.7 + 0.3 * i)
    return x.astype(np.complex64)


@functools.lru_cache(maxsize=None)
def _stream(seed, B, nb, T, L):
    x = _bursts(seed, B, nb, T, L)
    x.setflags(write=False)
    return x


def _plan(nb, T, L):
    return int(_lib.lib().ofs_aa_plan(_lib.C64, _lib.FP32, nb, T, L))


class _Ref:
    """The one-shot storing call on a whole stream (computed once per input, left unchanged)."""

    def __init__(self, x, L, hyst, fs=sync_aa.SAMPLE_RATE_HZ, thr=THR):
        B, nb, T = x.shape
        self.plan = _plan(nb, T, L)
        assert 1000 <= self.plan < 1200, self.plan
        assert (self.plan < 1100) == (T <= 1024 and T % 2 == 0), (self.plan, T)
        r = sync_aa.aa_detect_streaming_batched(torch.tensor(np.ascontiguousarray(x)).cuda(), L=L, threshold=thr,
                                                hysteresis=hyst, sample_rate=fs, precision="fp32", outputs=OUT,
                                                max_events=32)
        torch.cuda.synchronize()
        assert r.P.dtype == torch.complex64 and r.R.dtype == torch.float32
        self.r, self.n = r, r.n_events.cpu().numpy()
        assert self.n.max(initial=0) <= r.ev_int.shape[1]
        self.ev_int = [r.ev_int[b, :self.n[b]] for b in range(B)]
        self.ev_real = [r.ev_real[b, :self.n[b]] for b in range(B)]


@functools.lru_cache(maxsize=None)
def _ref(seed, B, nb, T, L, hyst):
    ref = _Ref(_stream(seed, B, nb, T, L), L, hyst)
    assert (ref.n >= 1).all(), ref.n                           # every stream opens and closes a gate
    return ref


def _bits(t):
    if t.dtype == torch.complex64:
        return torch.view_as_real(t).contiguous().view(torch.int32)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    return t


def _snap(r):
    """Clone of a push result, enqueued on the same stream (the detector reuses its buffers)."""
    return sync_aa.AABatchResult(*[None if t is None else t.clone() for t in
                                   (r.P, r.R, r.M, r.valid, r.n_events, r.ev_int, r.ev_real)])


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
        res.append(_snap(det.flush()))
    return res


def _events(res, b):
    n = [int(r.n_events[b]) for r in res]
    for r, k in zip(res, n):
        assert k <= r.ev_int.shape[1], (k, r.ev_int.shape)
    return (torch.cat([r.ev_int[b, :k] for r, k in zip(res, n)]), torch.cat([r.ev_real[b, :k] for r, k in zip(res, n)]),
            sum(n))


def _assert_events(res, ref, rows, what=""):
    for b in rows:
        ei, er, n = _events(res, b)
        assert n == ref.n[b], (what, b, n, ref.n[b])
        assert torch.equal(ei, ref.ev_int[b]), (what, b, ei.tolist(), ref.ev_int[b].tolist())
        assert torch.equal(_bits(er), _bits(ref.ev_real[b])), (what, b, er.tolist(), ref.ev_real[b].tolist())


def _assert_equal(res, ref, streams=None, what="", keys=OUT, nan_sign_free=False):
    """nan_sign_free (test_non_finite_head only): a word that is NaN in the one-shot result is compared
    without its sign bit - the NaN must be there, with the same payload."""
    B = ref.r.P.shape[0]
    rows = list(range(B)) if streams is None else list(streams)
    body = [r for r in res if r.R is not None]
    for k in keys:
        got = _bits(torch.cat([getattr(r, k) for r in body], dim=1))
        want = _bits(getattr(ref.r, k))
        if nan_sign_free and k != "valid":
            w = getattr(ref.r, k)
            nan = torch.isnan(torch.view_as_real(w) if w.is_complex() else w)
            got = torch.where(nan, got & 0x7fffffff, got)
            want = torch.where(nan, want & 0x7fffffff, want)
        if not torch.equal(got[rows], want[rows]):
            bad = (got[rows] != want[rows]).nonzero()
            raise AssertionError((what, k, "first differing [row, index(, part)]", bad[0].tolist(), "of", len(bad)))
    _assert_events(res, ref, rows, what)


def _detector(B, nb, L, hyst, **kw):
    kw.setdefault("outputs", OUT)
    kw.setdefault("max_events", 8)
    return sync_aa.AAChunkedDetectorF32(B, nb, L, threshold=THR, hysteresis=hyst, **kw)


def _rest(T, head):
    head = [c for c in head]
    assert sum(head) < T, (T, head)
    return head + [T - sum(head)]


def _chunkings(T, L):
    """One sample at a time across L; Tc < 128; Tc no multiple of 128; edges at L - 1, L, L + 1 and at
    a row boundary - 1, + 0, + 1; one chunk above 2L; the whole stream."""
    return [
        _rest(T, [L - 20] + [1] * 45),
        [100] * ((T - 1) // 100) + [T - 100 * ((T - 1) // 100)],
        [200] * ((T - 1) // 200) + [T - 200 * ((T - 1) // 200)],
        _rest(T, [L - 1, 1, 1, 126, 1, 1]),
        _rest(T, [10, 2 * L + 50]) if T > 2 * L + 61 else _rest(T, [T - 3]),
        [T],
    ]


# ------------------------------------------------------------------------------------------
# 1. splits
# ------------------------------------------------------------------------------------------
SPLITS = [  # (n_ant, L, T, hysteresis): per window length one even T <= 1024 (plan 10xx) and one odd T (plan 11xx)
    (1, 128, 1024, 16), (1, 128, 1111, 128), (2, 128, 1024, 128), (2, 128, 1111, 16),
    (1, 256, 1024, 16), (1, 256, 2 * 256 + 5 * 128 + 37, 16), (2, 256, 1024, 16), (2, 256, 2 * 256 + 5 * 128 + 37, 128),
    (2, 512, 2 * 512 + 5 * 128 + 37, 16),
]


@pytest.mark.parametrize("nb,L,T,hyst", SPLITS, ids=[f"na{c[0]}_L{c[1]}_T{c[2]}_h{c[3]}" for c in SPLITS])
def test_splits_equal_one_shot(nb, L, T, hyst):
    """B = 5 streams (more than the 4 of one workgroup), every chunking of _chunkings, the same detector
    throughout: each final call leaves fresh streams for the next chunking."""
    B, seed = 5, 1000 * nb + L + T
    ref = _ref(seed, B, nb, T, L, hyst)
    print("plan", ref.plan, "events per stream", ref.n.tolist())
    xt = torch.tensor(_stream(seed, B, nb, T, L)).cuda()
    det = _detector(B, nb, L, hyst)
    runs = []
    for i, chunks in enumerate(_chunkings(T, L)):
        assert sum(chunks) == T and min(chunks) >= 1
        runs.append((chunks, _feed(det, _cut(xt, chunks), final=True, flush=(i % 2 == 1))))
        assert det.samples_seen == 0
    torch.cuda.synchronize()
    for chunks, res in runs:
        _assert_equal(res, ref, what=f"chunks {chunks[:8]}...")


# ------------------------------------------------------------------------------------------
# 2. boundary sweep
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyst", [16, 128])
def test_boundary_sweep(hyst):
    """Every two-way split from L - 2 to L + 130 (the valid edge and a whole row behind it) and from two
    samples before a gate opens to two after it closes.  Hysteresis 16: the gate's scan rows, 128: its
    scan-free rows."""
    L, T, seed = 128, 1111, 77
    ref = _ref(seed, 1, 1, T, L, hyst)
    _, start, end, _ = ref.ev_int[0][0].tolist()
    assert end < T and end - start + 5 < 600, (start, end)
    cuts = sorted(set(range(L - 2, L + 131)) | set(range(max(start - 2, 1), min(end + 3, T))))
    xt = torch.tensor(_stream(seed, 1, 1, T, L)).cuda()
    det = _detector(1, 1, L, hyst)
    runs = [(s, _feed(det, [xt[:, :, :s].contiguous(), xt[:, :, s:].contiguous()], final=True)) for s in cuts]
    torch.cuda.synchronize()
    for s, res in runs:
        _assert_equal(res, ref, what=f"split {s}")


# ------------------------------------------------------------------------------------------
# 3. exact streams: |P|^2 ties, gates at row and stream edges
# ------------------------------------------------------------------------------------------
def _exact_cuts(orc, T, limit=48):
    """Chunk edges at the positions of exact |P|^2 ties: for every gate of every stream the positions
    that hold the gate's maximum (p and p + 1, so that two tied maxima fall into different calls), and
    the gate's start and end."""
    cuts, ties = set(), 0
    for P, R, M, valid, ei, er in orc:
        pm = P.real ** 2 + P.imag ** 2
        for peak, start, end, _ in ei:
            at = start + np.flatnonzero(pm[start:min(end, T - 1) + 1] == pm[peak])
            ties += len(at) > 1
            for p in list(at[:3]) + [start, end]:
                cuts |= {int(p), int(p) + 1}
    cuts = sorted(c for c in cuts if 1 <= c < T)
    step = max(1, len(cuts) // limit)
    return cuts[::step], ties


def _against_oracle(res, orc, L, what):
    """Events against ofdm_oracle.aa_detect on the same exact stream, no tie exemption: count, integers
    and P at the peak equal; M and the CFO within the fp32 paths' bounds of test_gpu_aa_exact_events.py
    (1e-6, and 1e-6 rad of angle)."""
    for b, (P, R, M, valid, ei, er) in enumerate(orc):
        gi, gr, n = _events(res, b)
        gi, gr = gi.cpu().numpy(), gr.cpu().numpy()
        assert n == len(ei), (what, b, n, len(ei))
        assert np.array_equal(gi, ei), (what, b, gi.tolist(), ei.tolist())
        assert np.array_equal(gr[:, :2], er[:, :2]), (what, b)
        if n:
            assert np.max(np.abs(gr[:, 2] - er[:, 2])) <= 1e-6, (what, b)
            assert np.max(np.abs(gr[:, 3] - er[:, 3])) <= 1e-6 * X.FS / (2 * np.pi * L), (what, b)


@pytest.mark.parametrize("L,T,nb", [(128, 1024, 1), (256, 1025, 2), (512, 2047, 1)], ids=str)
def test_exact_streams(L, T, nb):
    """The stream sets of tests/exact_streams.py as complex64, chunked at every row boundary and at the
    tie positions: equal to the one-shot call bit for bit and to the oracle's events."""
    total_ties = 0
    for hyst in (2, 16, 128, 257):
        names, iq = X.streams(L, T, hyst, nb)
        orc = X.oracle(L, T, hyst, nb)
        x = X.cplx(iq, np.complex64)
        B = len(names)
        ref = _Ref(x, L, hyst, fs=X.FS, thr=X.THR)
        cuts, ties = _exact_cuts(orc, T)
        total_ties += ties
        xt = torch.tensor(x).cuda()
        nmax = max(int(ref.n.max()), 1)
        det = sync_aa.AAChunkedDetectorF32(B, nb, L, threshold=X.THR, hysteresis=hyst, sample_rate=X.FS, outputs=OUT,
                                           max_events=nmax)
        rows = [128] * ((T - 1) // 128) + [T - 128 * ((T - 1) // 128)]
        at_ties = list(np.diff([0] + cuts + [T]))
        runs = [("rows", _feed(det, _cut(xt, rows))), ("ties", _feed(det, _cut(xt, at_ties), flush=True))]
        torch.cuda.synchronize()
        for name, res in runs:
            _assert_equal(res, ref, what=(name, L, T, hyst))
            _against_oracle(res, orc, L, (name, L, T, hyst))
    assert total_ties >= 1, "the stream sets hold gates with tied maxima"


# ------------------------------------------------------------------------------------------
# 4. gates carried over calls
# ------------------------------------------------------------------------------------------
def test_gate_open_over_three_calls():
    """Four chunk edges inside one gate: no event until the call that holds the close."""
    L, T, hyst, seed = 256, 1189, 16, 5
    ref = _ref(seed, 2, 1, T, L, hyst)
    peak, start, end, _ = ref.ev_int[0][0].tolist()
    assert end - start >= 12 and end < T
    q = (end - start) // 4
    cuts = [start + 1, start + q, start + 2 * q, start + 3 * q]
    chunks = list(np.diff([0] + cuts + [T]))
    xt = torch.tensor(_stream(seed, 2, 1, T, L)).cuda()
    res = _feed(_detector(2, 1, L, hyst), _cut(xt, chunks))
    torch.cuda.synchronize()
    assert [int(r.n_events[0]) for r in res[:4]] == [0, 0, 0, 0]
    assert int(res[4].n_events[0]) >= 1 and res[4].ev_int[0, 0].tolist() == [peak, start, end, peak - 2 * L + 1]
    _assert_equal(res, ref, what="gate over 5 calls")


def test_first_maximum_kept_on_a_tie_across_the_edge():
    """A gate whose maximum |P|^2 is held at p1 < p2 exactly (exact streams), split between them: the
    event comes from a later call and names p1."""
    L, T, hyst = 128, 1024, 16
    names, iq = X.streams(L, T, hyst, 1)
    orc = X.oracle(L, T, hyst, 1)
    x = X.cplx(iq, np.complex64)
    ref = _Ref(x, L, hyst, fs=X.FS, thr=X.THR)
    xt = torch.tensor(x).cuda()
    det = sync_aa.AAChunkedDetectorF32(len(names), 1, L, threshold=X.THR, hysteresis=hyst, sample_rate=X.FS, outputs=OUT,
                                       max_events=max(int(ref.n.max()), 1))
    found = []
    for b, (P, R, M, valid, ei, er) in enumerate(orc):
        pm = P.real ** 2 + P.imag ** 2
        for peak, start, end, _ in ei:
            at = start + np.flatnonzero(pm[start:min(end, T - 1) + 1] == pm[peak])
            if len(at) > 1 and at[0] == peak and at[-1] < T - 1:
                found.append((b, int(peak), int(at[-1])))
    assert found
    runs = []
    for b, p1, p2 in found[:6]:
        runs.append((b, p1, p2, _feed(det, _cut(xt, [p1 + 1, p2 - p1, T - p2 - 1]))))
    torch.cuda.synchronize()
    for b, p1, p2, res in runs:
        n0 = int(res[0].n_events[b])
        assert p1 not in res[0].ev_int[b, :n0, 0].tolist()      # the call that holds p1 does not report it yet
        ei, _, _ = _events(res, b)
        assert p1 in ei[:, 0].tolist(), (b, p1, p2, ei.tolist())
        _assert_equal(res, ref, what=("tie", b, p1, p2))


def test_flush_closes_at_samples_seen():
    """A stream that ends inside a gate: no event without final, flush() reports it with gate_end = the
    sample count (as the one-shot call closes it at T), and the streams are fresh afterwards."""
    L, hyst, seed = 128, 16, 9
    full = _stream(seed, 2, 1, 1111, L)
    peak = int(_ref(seed, 2, 1, 1111, L, hyst).ev_int[0][0, 0])
    T = peak + 5                                               # 5 samples past the peak: inside the gate
    x = np.ascontiguousarray(full[:, :, :T])
    ref = _Ref(x, L, hyst)
    assert ref.n[0] == 1 and int(ref.ev_int[0][0, 2]) == T
    xt = torch.tensor(x).cuda()
    pieces = _cut(xt, _rest(T, [T // 3, T // 3]))
    det = _detector(2, 1, L, hyst)
    first = _feed(det, pieces, final=False)
    assert det.samples_seen == T
    fl = _snap(det.flush())
    assert det.samples_seen == 0 and fl.P is None
    again = _feed(det, pieces, flush=True)
    torch.cuda.synchronize()
    assert sum(int(r.n_events[0]) for r in first) == 0         # still open: not reported
    assert int(fl.n_events[0]) == 1 and int(fl.ev_int[0, 0, 2]) == T
    _assert_equal(first + [fl], ref, what="first run")
    _assert_equal(again, ref, what="second run")


# ------------------------------------------------------------------------------------------
# 5. non-finite samples around L
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1024, 1111])
def test_non_finite_head(T):
    """NaN / Inf among the first L samples and right after L: P = M = +0.0 (all-zero bits) and valid = 0
    for n < L whatever the samples are, and everything equals the one-shot call: every word that is not
    a NaN there bit for bit, every NaN word a NaN with the same payload, and the events.

    The SIGN of a NaN word is left out, because the yardstick does not define it: on the same samples
    (this test's streams, 1026 samples, and their first 1024) aa_fast_kernel and aa_stream_kernel return
    the same 8432 NaN words of P in the same places, but 64 of them (imaginary part, row 3 of the
    stream with x[L] = NaN j) are 0xffc00000 from the first and 0x7fc00000 from the second, where two
    NaNs of opposite sign meet in one add and the operand order is the compiler's; the chunked kernel
    had the first kernel's bits in all 8432.  A chunked call cannot know T, so it cannot follow both."""
    L, hyst, B = 128, 16, 5
    x = _stream(21, B, 1, T, L).copy()
    x[0, 0, 5] = np.nan
    x[1, 0, 100] = complex(np.inf, 0)
    x[2, 0, L] = complex(0, np.nan)
    x[3, 0, L + 1] = complex(-np.inf, 1)
    x[4, 0, 3] = np.nan
    x[4, 0, L - 1] = complex(1, -np.inf)
    ref = _Ref(x, L, hyst)
    xt = torch.tensor(x).cuda()
    det = _detector(B, 1, L, hyst)
    runs = [_feed(det, _cut(xt, c)) for c in (_rest(T, [50, 78, 1, 1]), _rest(T, [3] * 60), [T])]
    torch.cuda.synchronize()
    for res in runs:
        P = torch.cat([r.P for r in res], dim=1)
        M = torch.cat([r.M for r in res], dim=1)
        V = torch.cat([r.valid for r in res], dim=1)
        assert not bool(_bits(P)[:, :L].any()) and not bool(_bits(M)[:, :L].any()) and not bool(V[:, :L].any())
        assert bool(V[:, L:].all())
        _assert_equal(res, ref, what="non-finite", nan_sign_free=True)


# ------------------------------------------------------------------------------------------
# 6. other behaviour
# ------------------------------------------------------------------------------------------
def test_per_stream_reset():
    """reset(mask) after two chunks: the reset streams continue as a one-shot call on the remaining
    samples (indices from 0, rows aligned to the new start), the others are unaffected."""
    B, nb, T, L, hyst, seed = 4, 1, 1701, 128, 16, 41
    chunks = [300, 277, T - 577]
    ref = _ref(seed, B, nb, T, L, hyst)
    x = _stream(seed, B, nb, T, L)
    tail = _Ref(np.ascontiguousarray(x[:, :, 577:]), L, hyst)
    assert tail.n[0] >= 1
    pieces = _cut(torch.tensor(x).cuda(), chunks)
    det = _detector(B, nb, L, hyst)
    res = _feed(det, pieces[:2], final=False)
    det.reset(torch.tensor([True, True, False, False]))
    res += _feed(det, pieces[2:], final=True)
    torch.cuda.synchronize()
    _assert_equal(res, ref, streams=(2, 3), what="kept")
    _assert_equal(res[2:], tail, streams=(0, 1), what="reset")
    det.push(pieces[0])
    det.reset()
    assert det.samples_seen == 0 and not bool(det.state.any())


def test_event_overflow_keeps_exact_count():
    """max_events = 1 with several gates closing in one call: the count stays exact and slot 0 holds
    the first event."""
    L, hyst, T, seed = 128, 16, 1701, 41
    ref = _ref(seed, 4, 1, T, L, hyst)
    assert ref.n[0] >= 2
    det = _detector(4, 1, L, hyst, max_events=1)
    r = _snap(det.push(torch.tensor(_stream(seed, 4, 1, T, L)).cuda(), final=True))
    torch.cuda.synchronize()
    assert r.ev_int.shape[1] == 1
    for b in range(4):
        assert int(r.n_events[b]) == ref.n[b]
        assert torch.equal(r.ev_int[b, 0], ref.ev_int[b][0])
        assert torch.equal(_bits(r.ev_real[b, 0]), _bits(ref.ev_real[b][0]))


def test_chunks_enqueued_without_host_synchronisation():
    """All chunks enqueued back to back ([B, Tc] input for one antenna, uploaded beforehand, each result
    cloned on the same stream), one synchronisation at the end."""
    B, T, L, hyst, seed = 5, 1111, 128, 128, 1000 + 128 + 1111
    ref = _ref(seed, B, 1, T, L, hyst)
    xt = torch.tensor(_stream(seed, B, 1, T, L)).cuda()
    pieces = [p[:, 0].contiguous() for p in _cut(xt, [97] * 11 + [T - 97 * 11])]
    det = _detector(B, 1, L, hyst)
    torch.cuda.synchronize()
    res = []
    for i, p in enumerate(pieces):                             # nothing below waits for the GPU
        res.append(_snap(det.push(p, final=i == len(pieces) - 1)))
    torch.cuda.synchronize()
    _assert_equal(res, ref, what="back to back")


def test_events_only_equals_the_storing_run():
    """outputs=(): no P/R/M/valid buffers, the same arithmetic - the events of the storing chunked run
    (and so of the one-shot storing call)."""
    B, nb, T, L, hyst, seed = 5, 2, 1111, 128, 16, 2000 + 128 + 1111
    ref = _ref(seed, B, nb, T, L, hyst)
    xt = torch.tensor(_stream(seed, B, nb, T, L)).cuda()
    chunks = _rest(T, [131, 1, 300, 64])
    stored = _feed(_detector(B, nb, L, hyst), _cut(xt, chunks))
    only = _feed(_detector(B, nb, L, hyst, outputs=()), _cut(xt, chunks))
    torch.cuda.synchronize()
    assert all(r.P is None and r.R is None and r.M is None and r.valid is None for r in only)
    for b in range(B):
        (si, sr, sn), (oi, orl, on) = _events(stored, b), _events(only, b)
        assert sn == on and torch.equal(si, oi) and torch.equal(_bits(sr), _bits(orl)), b
    _assert_events(only, ref, range(B), "events only")


# ------------------------------------------------------------------------------------------
# 7. longer than a toy
# ------------------------------------------------------------------------------------------
def test_long_stream_uneven_pieces():
    """About 20 000 samples, two antennas, L = 512 (156 rows: the carried fp64 bases are sums over
    the whole stream by the end), in uneven pieces."""
    B, nb, T, L, hyst, seed = 2, 2, 20011, 512, 128, 3
    ref = _ref(seed, B, nb, T, L, hyst)
    assert ref.plan == 1124
    xt = torch.tensor(_stream(seed, B, nb, T, L)).cuda()
    chunks = _rest(T, [1000, 37, 4096, 511, 513, 1, 5000, 129, 2048, 3000])
    res = _feed(_detector(B, nb, L, hyst), _cut(xt, chunks))
    torch.cuda.synchronize()
    _assert_equal(res, ref, what="long")
