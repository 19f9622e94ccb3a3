"""Resumable chunked [A][A] detection (csrc/aa_chunk.hip, sync_aa.AAChunkedDetector).

For int16 / packed 12-bit input every window sum is an exact integer, so ANY chunking of a stream
must reproduce the one-shot call bit for bit: the concatenated P, R, M, valid and the sequence of
events (absolute indices).  The reference of every case is the one-shot
``aa_detect_streaming_batched`` on the whole stream (integer-exact plan 2000-2999), compared with
``torch.equal``; streams 0 and B-1 are also checked against the CPU oracle (P, R, valid exactly,
|dM| < 1e-12 as in test_gpu_exact.py).  Past the one-shot plan's reach the oracle is the reference.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import ofdm_oracle as O
import oracle_c

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ofdm_sync_amd import _lib, sync_aa, wire  # noqa: E402

THR = 0.15
OUT = ("P", "R", "M", "valid")


def _int12_bursts(rng, B, nb, T, blocks, amp=1500, noise=60):
    """int16 I/Q [B, nb, T, 2]: int12 noise plus, in every other stream, a burst made of the
    given block pattern (e.g. [1, 1] for [A][A]) of a random segment (tests/test_gpu_exact.py)."""
    x = rng.normal(0, noise, (B, nb, T)) + 1j * rng.normal(0, noise, (B, nb, T))
    seg = len(blocks[1])
    for b in range(0, B, 2):
        n = seg * len(blocks[0])
        if T > n + 2:
            s = int(rng.integers(0, T - n))
            a = rng.normal(0, amp / 3, seg) + 1j * rng.normal(0, amp / 3, seg)
            burst = np.concatenate([sgn * a for sgn in blocks[0]])
            x[b, :, s:s + n] += burst
    re = np.clip(np.round(x.real), -2048, 2047)
    im = np.clip(np.round(x.imag), -2048, 2047)
    return np.stack([re, im], axis=-1).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _stream(seed, B, nb, T, L):
    iq = _int12_bursts(np.random.default_rng(seed), B, nb, T, ([1, 1], np.zeros(L)))
    iq.setflags(write=False)
    return iq


class _Ref:
    """One-shot result of a whole stream (computed once per input, left unchanged)."""

    def __init__(self, iq, L, hyst):
        B, nb, T, _ = iq.shape
        plan = _lib.lib().ofs_aa_plan(_lib.CI16, _lib.FP64, nb, T, L)
        assert 2000 <= plan <= 2999, plan                      # the integer-exact one-shot kernel
        r = sync_aa.aa_detect_streaming_batched(torch.tensor(iq).cuda(), L=L, threshold=THR, hysteresis=hyst,
                                                outputs=OUT, max_events=16)
        torch.cuda.synchronize()
        self.r, self.n = r, r.n_events.cpu().numpy()
        self.ev_int = [r.ev_int[b, :self.n[b]] for b in range(B)]
        self.ev_real = [r.ev_real[b, :self.n[b]] for b in range(B)]


@functools.lru_cache(maxsize=None)
def _ref(seed, B, nb, T, L, hyst):
    ref = _Ref(_stream(seed, B, nb, T, L), L, hyst)
    assert (ref.n[::2] >= 1).all(), ref.n                      # every burst stream opens a gate
    return ref


def _pieces(iq, chunks, cp12):
    """Device tensors of the consecutive chunks (int16 [B, nb, Tc, 2] or AXIS words [B, Tc, 3 nb])."""
    out, s = [], 0
    for c in chunks:
        part = np.ascontiguousarray(iq[:, :, s:s + c])
        out.append(torch.tensor(wire.pack_axis(part) if cp12 else part).cuda())
        s += c
    assert s == iq.shape[2]
    return out


def _snap(r):
    """Clone of a push result, enqueued on the same stream (the detector reuses its buffers)."""
    return sync_aa.AABatchResult(*[None if t is None else t.clone() for t in
                                   (r.P, r.R, r.M, r.valid, r.n_events, r.ev_int, r.ev_real)])


def _feed(det, pieces, final=True, flush=False):
    """Push the pieces back to back without any host synchronisation."""
    res = [_snap(det.push(p, final=final and not flush and i == len(pieces) - 1)) for i, p in enumerate(pieces)]
    if flush:
        res.append(_snap(det.flush()))
    return res


def _events(res, b):
    n = [int(r.n_events[b]) for r in res]
    for r, k in zip(res, n):
        assert k <= r.ev_int.shape[1]
    return (torch.cat([r.ev_int[b, :k] for r, k in zip(res, n)]), torch.cat([r.ev_real[b, :k] for r, k in zip(res, n)]),
            sum(n))


def _assert_equal(res, ref, streams=None, what=""):
    B = ref.r.P.shape[0]
    rows = list(range(B)) if streams is None else list(streams)
    body = [r for r in res if r.P is not None]
    for k in OUT:
        got = torch.cat([getattr(r, k) for r in body], dim=1)
        assert torch.equal(got[rows], getattr(ref.r, k)[rows]), (what, k)
    for b in rows:
        ei, er, n = _events(res, b)
        assert n == ref.n[b], (what, b, n, ref.n[b])
        assert torch.equal(ei, ref.ev_int[b]), (what, b, ei, ref.ev_int[b])
        assert torch.equal(er, ref.ev_real[b]), (what, b, er, ref.ev_real[b])


def _assert_oracle(res, iq, L, streams):
    for b in streams:
        xc = (iq[b, ..., 0] + 1j * iq[b, ..., 1]).astype(np.complex128)
        P, R, M, v = O.aa_metric(xc, L)
        got = {k: torch.cat([getattr(r, k)[b] for r in res if r.P is not None]).cpu().numpy() for k in OUT}
        assert np.array_equal(got["P"], P)
        assert np.array_equal(got["R"], R)
        assert np.array_equal(got["valid"], v)
        assert np.max(np.abs(got["M"] - M)) < 1e-12


def _detector(B, nb, L, hyst, cp12=False, **kw):
    return sync_aa.AAChunkedDetector(B, nb, L, threshold=THR, hysteresis=hyst, in_dtype="cp12" if cp12 else torch.int16,
                                     outputs=OUT, **kw)


def _rest(T, head):
    return list(head) + [T - sum(head)]


SPLITS = [
    (5, 1, 3000, 64, 16, [500] * 6),
    (4, 2, 2999, 128, 16, _rest(2999, [1, 127, 128, 129, 255, 256, 257, 1000])),
    (3, 1, 6000, 512, 128, [1024] * 5 + [880]),
    (3, 2, 5000, 256, 300, _rest(5000, [64] * 20)),
    (2, 1, 9000, 1024, 1, _rest(9000, [2048, 2047, 2049])),
]
SPLIT_CASES = [(c, False) for c in SPLITS] + [(c, True) for c in SPLITS[:3]]


@pytest.mark.parametrize("case,cp12", SPLIT_CASES,
                         ids=[f"B{c[0]}_na{c[1]}_T{c[2]}_L{c[3]}_h{c[4]}_{'cp12' if p else 'ci16'}" for c, p in SPLIT_CASES])
def test_splits_equal_one_shot(case, cp12):
    """1. Any chunking equals the one-shot call; hysteresis 1 / 16 take the gate's scan path,
    128 / 300 the scan-free path (H >= one row).  The last chunk final, or not final + flush()."""
    B, nb, T, L, hyst, chunks = case
    assert sum(chunks) == T and min(chunks) >= 1
    iq, ref = _stream(B * 7 + L, B, nb, T, L), _ref(B * 7 + L, B, nb, T, L, hyst)
    pieces = _pieces(iq, chunks, cp12)
    det = _detector(B, nb, L, hyst, cp12)
    res = _feed(det, pieces, final=True)
    assert det.samples_seen == 0
    res2 = _feed(det, pieces, flush=True)                      # the final call left fresh streams
    torch.cuda.synchronize()
    _assert_equal(res, ref, what="final")
    _assert_equal(res2, ref, what="flush")
    _assert_oracle(res, iq, L, (0, B - 1))


@pytest.mark.parametrize("L", [64, 128])
@pytest.mark.parametrize("hyst", [16, 128])
def test_boundary_sweep(L, hyst):
    """2. Every two-way split within 2 samples of a gate's start, peak, last above-threshold sample
    and end, and at the valid / history edges: gates that open in one call and close in the next, a
    close on the first and on the last sample of a chunk, a peak in an earlier call than its event."""
    T = 1500 + 4 * L
    seed = 100 + L
    iq, ref = _stream(seed, 1, 1, T, L), _ref(seed, 1, 1, T, L, hyst)
    cuts = {1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, T - 1}
    for peak, start, end, _ in ref.ev_int[0].cpu().numpy():
        for g in (start, peak, end, end - max(hyst, 1)):
            cuts |= set(range(int(g) - 2, int(g) + 3))
    cuts = sorted(s for s in cuts if 1 <= s <= T - 1)
    assert len(cuts) >= 20
    xt = torch.tensor(iq).cuda()
    det = _detector(1, 1, L, hyst)
    runs = [(s, _feed(det, [xt[:, :, :s], xt[:, :, s:]], final=True)) for s in cuts]
    torch.cuda.synchronize()
    for s, res in runs:
        _assert_equal(res, ref, what=f"split {s}")


def test_open_gate_is_carried_until_flush():
    """3. A stream that ends inside a gate: no event without final, flush() reports it with
    gate_end == T, and the state is fresh afterwards."""
    L, hyst = 64, 16
    full = _stream(31, 2, 1, 2000, L)
    peak = int(_ref(31, 2, 1, 2000, L, hyst).ev_int[0][0, 0])
    T = peak + 5                                               # 5 samples past the peak: inside the gate
    iq = np.ascontiguousarray(full[:, :, :T])
    ref = _Ref(iq, L, hyst)
    assert ref.n[0] == 1 and int(ref.ev_int[0][0, 2]) == T   # the one-shot call closes it at T
    chunks = _rest(T, [T // 3, T // 3])
    pieces = _pieces(iq, chunks, False)
    det = _detector(2, 1, L, hyst)
    first = _feed(det, pieces, final=False)
    assert det.samples_seen == T
    fl = _snap(det.flush())
    again = _feed(det, pieces, final=False) + [_snap(det.flush())]
    torch.cuda.synchronize()
    assert sum(int(r.n_events[0]) for r in first) == 0         # still open: not reported
    assert int(fl.n_events[0]) == 1 and int(fl.ev_int[0, 0, 2]) == T
    _assert_equal(first + [fl], ref, what="first run")
    _assert_equal(again, ref, what="second run")


def test_per_stream_reset():
    """4. reset(mask) after two chunks: the reset streams continue as a one-shot call on the
    remaining samples (indices from 0), the others are unaffected."""
    B, nb, T, L, hyst = 4, 1, 3000, 64, 16
    chunks = [500, 700, 1800]
    iq, ref = _stream(41, B, nb, T, L), _ref(41, B, nb, T, L, hyst)
    tail = _Ref(np.ascontiguousarray(iq[:, :, 1200:]), L, hyst)
    assert tail.n[0] >= 1                                      # a reset burst stream still finds its gate
    pieces = _pieces(iq, chunks, False)
    det = _detector(B, nb, L, hyst)
    res = _feed(det, pieces[:2], final=False)
    det.reset(torch.tensor([True, True, False, False]))
    res += _feed(det, pieces[2:], final=True)
    torch.cuda.synchronize()
    _assert_equal(res, ref, streams=(2, 3), what="kept")
    _assert_equal(res[2:], tail, streams=(0, 1), what="reset")
    det.reset()
    assert det.samples_seen == 0 and not bool(det.state.any())


def test_past_the_one_shot_limit():
    """5. A stream longer than the integer-exact one-shot plan reaches, against the C oracle."""
    B, L, hyst = 2, 512, 128
    T = (1 << 21) + 3 * 4096
    assert not 2000 <= _lib.lib().ofs_aa_plan(_lib.CI16, _lib.FP64, 1, T, L) <= 2999
    rng = np.random.default_rng(5)
    iq = np.empty((B, 1, T, 2), np.int16)
    for s in range(0, T, 1 << 19):                             # int12 noise, generated in pieces
        n = min(1 << 19, T - s)
        iq[:, :, s:s + n] = np.clip(np.round(rng.normal(0, 60, (B, 1, n, 2))), -2048, 2047)
    a = np.round(rng.normal(0, 500, L) + 1j * rng.normal(0, 500, L))
    s0 = T - 6000                                              # [A][A] in the last 10000 samples of stream 0
    iq[0, 0, s0:s0 + 2 * L, 0] = np.clip(iq[0, 0, s0:s0 + 2 * L, 0] + np.tile(a.real, 2), -2048, 2047)
    iq[0, 0, s0:s0 + 2 * L, 1] = np.clip(iq[0, 0, s0:s0 + 2 * L, 1] + np.tile(a.imag, 2), -2048, 2047)
    chunks = [1 << 18] * (T >> 18) + [T % (1 << 18)]
    xt = torch.from_numpy(iq).cuda()
    det = _detector(B, 1, L, hyst)
    res, s = [], 0
    for i, c in enumerate(chunks):
        res.append(_snap(det.push(xt[:, :, s:s + c], final=i == len(chunks) - 1)))
        s += c
    torch.cuda.synchronize()
    want = oracle_c.aa_detect(iq[..., 0].astype(np.float64) + 1j * iq[..., 1], L, threshold=THR, hysteresis=hyst,
                              sample_rate=sync_aa.SAMPLE_RATE_HZ)
    P = torch.cat([r.P for r in res], dim=1).cpu().numpy()
    R = torch.cat([r.R for r in res], dim=1).cpu().numpy()
    M = torch.cat([r.M for r in res], dim=1).cpu().numpy()
    assert np.array_equal(P, want["P"])
    # R: exactly the integer window sums (the NumPy oracle's integer prefixes, < 2^53).  The C oracle
    # follows the reference's |x|^2 = hypot(I, Q)^2, which is not an integer for every word (its R is
    # off the integer sum by 1.8e-12 already on a 3000-sample stream), and keeps that in a running sum:
    # up to L terms in the window, each within 4 ulp of <= 2^23, plus one rounding of the sum per added
    # and per removed term over T samples
    for b in range(B):
        Po, Ro, _, _ = O.aa_metric(iq[b, 0, :, 0].astype(np.float64) + 1j * iq[b, 0, :, 1], L)
        assert np.array_equal(P[b], Po)
        assert np.array_equal(R[b], Ro)
    dR = float(np.max(np.abs(R - want["R"])))
    print("max |dR| vs the C oracle's running sum:", dR)
    assert dR <= 4 * L * np.spacing(2.0 ** 23) + 2 * T * np.spacing(float(R.max())) / 2
    dM = float(np.max(np.abs(M - want["M"])))
    print("max |dM| vs the C oracle:", dM)
    assert dM < 1e-12
    peaks = []
    for b in range(B):
        ei, er, n = _events(res, b)
        ei, er = ei.cpu().numpy(), er.cpu().numpy()
        wi, wr = want["ev_int"][b, :want["n_events"][b]], want["ev_real"][b, :want["n_events"][b]]
        print("stream", b, "events", ei.tolist(), "real diff", (er - wr).tolist() if n == len(wr) else None)
        assert n == want["n_events"][b]
        assert np.array_equal(ei, wi)
        assert np.array_equal(er[:, :2], wr[:, :2])            # P at the peak: exact integers
        # M at the peak: the M bound above.  CFO = atan2(P) * fs / (2 pi L) of the same exact P: two
        # atan2 implementations within 2 ulp of an angle <= pi each, then two roundings each of a result
        # <= fs / (2 L): 4 ulp(pi) * fs / (2 pi L) + 4 ulp(fs / (2 L)), ~1.6e-11 Hz
        scale = sync_aa.SAMPLE_RATE_HZ / (2 * np.pi * L)
        assert np.all(np.abs(er[:, 2] - wr[:, 2]) < 1e-12)
        assert np.all(np.abs(er[:, 3] - wr[:, 3]) <= 4 * np.spacing(np.pi) * scale + 4 * np.spacing(np.pi * scale))
        peaks += ei[:, 0].tolist()
    assert peaks and max(peaks) > (1 << 21)


def test_event_overflow_keeps_exact_count():
    """6. max_events = 1 with two gates closing in one call: the count stays exact and slot 0 holds
    the first event."""
    L, hyst, T = 64, 16, 3000
    rng = np.random.default_rng(7)
    x = rng.normal(0, 60, (1, 1, T)) + 1j * rng.normal(0, 60, (1, 1, T))
    for s in (600, 1900):
        a = rng.normal(0, 500, L) + 1j * rng.normal(0, 500, L)
        x[0, 0, s:s + 2 * L] += np.tile(a, 2)
    iq = np.stack([np.clip(np.round(x.real), -2048, 2047), np.clip(np.round(x.imag), -2048, 2047)], -1).astype(np.int16)
    ref = _Ref(iq, L, hyst)
    assert ref.n[0] == 2
    det = _detector(1, 1, L, hyst, max_events=1)
    r = _snap(det.push(torch.from_numpy(iq).cuda(), final=True))
    torch.cuda.synchronize()
    assert int(r.n_events[0]) == 2
    assert torch.equal(r.ev_int[0, 0], ref.ev_int[0][0]) and torch.equal(r.ev_real[0, 0], ref.ev_real[0][0])


def test_chunks_enqueued_without_host_synchronisation():
    """7. All chunks of the first split shape enqueued back to back (inputs uploaded beforehand, each
    result cloned on the same stream), one synchronisation at the end."""
    B, nb, T, L, hyst, chunks = SPLITS[0]
    iq, ref = _stream(B * 7 + L, B, nb, T, L), _ref(B * 7 + L, B, nb, T, L, hyst)
    pieces = _pieces(iq, chunks, False)
    det = _detector(B, nb, L, hyst)
    torch.cuda.synchronize()
    res = []
    for i, p in enumerate(pieces):                             # nothing below waits for the GPU
        res.append(_snap(det.push(p, final=i == len(pieces) - 1)))
    torch.cuda.synchronize()
    _assert_equal(res, ref, what="back to back")


def test_chunk_above_limit_names_it():
    det = _detector(1, 2, 1024, 16)
    assert det.max_chunk == (1 << 20) - 2048
    with pytest.raises(ValueError, match=str(det.max_chunk)):
        det.push(torch.zeros((1, 2, det.max_chunk + 1, 2), dtype=torch.int16, device="cuda"))
