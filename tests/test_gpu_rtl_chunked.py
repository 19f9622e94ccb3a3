"""Resumable chunked minn_rtl detection (csrc/rtl_chunk.hip, minn_rtl.MinnRTLChunkedDetector).

For int16 / packed 12-bit input every product and window sum is an exact integer and the IIR state is
carried exactly, so ANY chunking of a stream must reproduce the one-shot call bit for bit: the eight
concatenated arrays, the sequence of events (absolute indices) and the last call's open_gate_start.
The reference of every case is the one-shot ``minn_rtl_batched`` on the whole stream (integer-exact
plan 2000-2999), compared with ``torch.equal``; two streams per case are also checked against the
CPU oracle with ``np.array_equal``.  Past the one-shot plan's reach the C oracle is the reference.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import pytest

import ofdm_oracle as O
import oracle_c

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ofdm_sync_amd import _lib, minn_rtl, wire  # noqa: E402

KEYS = ("corr_total", "corr_positive", "smooth_metric", "energy_total", "corr_scaled", "energy_scaled",
        "metric_valid", "above_threshold")
THR, THR12, FRAC, TOFF = 3276, 30, 15, -5
MAX_EV = 64


def _int12_bursts(rng, B, nb, T, blocks, amp=1500, noise=60):
    """int16 I/Q [B, nb, T, 2]: int12 noise plus, in every other stream, a burst made of the given
    block pattern ([1, 1, -1, -1] for Minn) of a random segment (tests/test_gpu_aa_chunked.py)."""
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
def _stream(seed, B, nb, T, Q):
    iq = _int12_bursts(np.random.default_rng(seed), B, nb, T, ([1, 1, -1, -1], np.zeros(Q)))
    iq.setflags(write=False)
    return iq


def _par(mode="float", shift=3, hyst=2, toff=TOFF):
    """Threshold 3276 / 2^15 = 0.1 of the energy, the package default.  With shift 12 the smoothed
    metric has a time constant of 4096 samples: over a 4Q <= 512-sample burst it reaches at most a few
    per cent of the burst's correlation, so 0.1 can never fire; 30 / 2^15 = 0.0009 lies between what the
    noise reaches (corr_positive of noise is ~0.03 of the energy and has had ~T/4096 of its rise) and
    what a burst reaches, and every burst stream gets its event (asserted in _ref)."""
    return dict(smooth_shift=shift, threshold_value=THR12 if shift == 12 else THR, threshold_frac_bits=FRAC,
                smooth_mode=mode, hysteresis=hyst, timing_offset=toff)


class _Ref:
    """One-shot result of a whole stream on the integer-exact plan (computed once, left unchanged)."""

    def __init__(self, iq, Q, par):
        B, nb, T, _ = iq.shape
        plan = _lib.lib().ofs_rtl_plan(_lib.CI16, nb, T, Q)
        assert 2000 <= plan <= 2999, plan
        r = minn_rtl.minn_rtl_batched(torch.tensor(iq).cuda(), Q, max_events=MAX_EV, **par)
        torch.cuda.synchronize()
        self.r, self.n = r, r.n_events.cpu().numpy()
        assert self.n.max() <= r.events.shape[1]
        self.events = [r.events[b, :self.n[b]] for b in range(B)]
        self.open = r.open_gate_start


@functools.lru_cache(maxsize=None)
def _ref(seed, B, nb, T, Q, mode, shift, hyst):
    ref = _Ref(_stream(seed, B, nb, T, Q), Q, _par(mode, shift, hyst))
    assert (ref.n[::2] >= 1).all(), ref.n                      # every burst stream has an event
    return ref


def _pieces(iq, chunks, cp12=False):
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
    return dataclasses.replace(r, **{f.name: (None if getattr(r, f.name) is None else getattr(r, f.name).clone())
                                     for f in dataclasses.fields(r)})


def _feed(det, pieces, final=True, flush=False):
    """Push the pieces back to back without any host synchronisation."""
    res = [_snap(det.push(p, final=final and not flush and i == len(pieces) - 1)) for i, p in enumerate(pieces)]
    if flush:
        res.append(_snap(det.flush()))
    return res


def _events(res, b):
    n = [int(r.n_events[b]) for r in res]
    for r, k in zip(res, n):
        assert k <= r.events.shape[1]
    return torch.cat([r.events[b, :k] for r, k in zip(res, n)]), sum(n)


def _assert_equal(res, ref, streams=None, what=""):
    B = ref.r.corr_total.shape[0]
    rows = list(range(B)) if streams is None else list(streams)
    body = [r for r in res if r.corr_total is not None]
    for k in KEYS:
        got = torch.cat([getattr(r, k) for r in body], dim=1)
        assert torch.equal(got[rows], getattr(ref.r, k)[rows]), (what, k)
    for b in rows:
        ev, n = _events(res, b)
        assert n == ref.n[b], (what, b, n, ref.n[b])
        assert torch.equal(ev, ref.events[b]), (what, b, ev, ref.events[b])
    assert torch.equal(res[-1].open_gate_start[rows], ref.open[rows]), (what, res[-1].open_gate_start, ref.open)


def _assert_oracle(res, iq, Q, par, streams):
    for b in streams:
        xc = (iq[b, ..., 0] + 1j * iq[b, ..., 1]).astype(np.complex128)
        s = O.minn_rtl_metric(xc, Q, par["smooth_shift"], par["threshold_value"], FRAC, smooth_mode=par["smooth_mode"])
        for k in KEYS:
            got = torch.cat([getattr(r, k)[b] for r in res if r.corr_total is not None]).cpu().numpy()
            assert np.array_equal(got, s[k]), (b, k)
        ev, segs, _ = O.detect_minn_rtl(s["corr_positive"], s["above_threshold"], s["metric_valid"],
                                        par["hysteresis"], par["timing_offset"])
        got, _ = _events(res, b)
        assert np.array_equal(got.cpu().numpy(), ev), (b, got, ev)
        want_open = int(segs[-1, 0]) if len(segs) > len(ev) else -1       # the open gate is the extra segment
        assert int(res[-1].open_gate_start[b]) == want_open, (b, res[-1].open_gate_start[b], want_open)


def _detector(B, nb, Q, par, cp12=False, **kw):
    kw.setdefault("max_events", MAX_EV)
    return minn_rtl.MinnRTLChunkedDetector(B, Q, nb, in_dtype="cp12" if cp12 else torch.int16, **par, **kw)


def _rest(T, head):
    return list(head) + [T - sum(head)]


def _both_passes(iq, ref, Q, par, chunks, cp12=False, oracle=(), what=""):
    """The chunking once with a final last push and once with a non-final last push + flush(): the
    second pass proves the first left fresh streams."""
    B, nb = iq.shape[:2]
    pieces = _pieces(iq, chunks, cp12)
    det = _detector(B, nb, Q, par, cp12)
    res = _feed(det, pieces, final=True)
    assert det.samples_seen == 0
    res2 = _feed(det, pieces, flush=True)
    torch.cuda.synchronize()
    _assert_equal(res, ref, what=what + " final")
    _assert_equal(res2, ref, what=what + " flush")
    assert int(res2[-1].n_events.sum()) == 0                   # a flush reports no event
    if oracle:
        _assert_oracle(res, iq, Q, par, oracle)


SPLITS = [
    (5, 1, 3000, 64, 2, [500] * 6),
    (4, 2, 2999, 128, 0, _rest(2999, [1, 127, 128, 129, 255, 256, 257, 383, 385])),
    (3, 1, 9000, 512, 40, [1024] * 8 + [808]),
    (3, 2, 5000, 256, 300, _rest(5000, [64] * 20)),
]
SPLIT_CASES = ([(c, False, "float", 3) for c in SPLITS] + [(c, True, "float", 3) for c in SPLITS[:3]] +
               [(c, False, m, s) for c in SPLITS[:2] for m, s in (("floor", 3), ("float", 0), ("float", 12),
                                                                 ("floor", 0), ("floor", 12))])


@pytest.mark.parametrize("case,cp12,mode,shift", SPLIT_CASES,
                         ids=[f"B{c[0]}_nb{c[1]}_T{c[2]}_Q{c[3]}_h{c[4]}_{'cp12' if p else 'ci16'}_{m}{s}"
                              for c, p, m, s in SPLIT_CASES])
def test_splits_equal_one_shot(case, cp12, mode, shift):
    """1. Any chunking equals the one-shot call: hysteresis 0 / 2 / 40 take the gate's scan path, 300
    the scan-free path (H >= one 256-sample gate row); float and floor smoothing, shift 0 / 3 / 12."""
    B, nb, T, Q, hyst, chunks = case
    assert sum(chunks) == T and min(chunks) >= 1
    seed = B * 7 + Q
    iq, ref = _stream(seed, B, nb, T, Q), _ref(seed, B, nb, T, Q, mode, shift, hyst)
    _both_passes(iq, ref, Q, _par(mode, shift, hyst), chunks, cp12, oracle=(0, B - 1))


EDGES = (1, 62, 63, 64, 127, 128, 190, 191, 192, 255, 256, 257)


@pytest.mark.parametrize("mode", ["float", "floor"])
def test_chunk_edge_in_the_fill_phase_and_on_row_and_segment_boundaries(mode):
    """2. Q = 64: the first edge on every tap's first valid sample (Q-1, 2Q-1, 3Q-1), on row (64) and
    segment (256) boundaries and next to them; the second chunk's END takes the same values mod 256."""
    Q, T, B, hyst = 64, 1400, 4, 2
    iq, ref = _stream(21, B, 1, T, Q), _ref(21, B, 1, T, Q, mode, 3, hyst)
    for j, c1 in enumerate(EDGES):
        end2 = 512 + EDGES[(j + 5) % len(EDGES)]
        assert end2 % 256 == EDGES[(j + 5) % len(EDGES)] % 256 and c1 < end2 < T
        _both_passes(iq, ref, Q, _par(mode, 3, hyst), [c1, end2 - c1, T - end2], oracle=(0,) if j == 0 else (),
                     what=f"c1={c1} end2={end2}")


@pytest.mark.parametrize("mode", ["float", "floor"])
@pytest.mark.parametrize("chunks", [[500, 200, 130, 370], [292, 408, 130, 370]], ids=["in_plateau", "plateau_start"])
def test_tie_rule_across_calls_on_an_exact_plateau(mode, chunks):
    """3. corr_positive sits on its maximum 128000000 over [291, 699]: the peak is the LAST maximum,
    699, also when the plateau is cut by a chunk edge (a strict > in the carry merge would report 499
    or 291), when the peak is the last sample of a chunk (699), when the gate closes on the last sample
    of a chunk (829) and with a new gate left open at the end (the all-zero tail is above: 0 >= 0)."""
    Q, T = 64, 1200
    par = _par(mode, 3, 2, toff=0)
    x = np.zeros(T, np.complex128)
    x[100:700] = 1000.0
    s = O.minn_rtl_metric(x, Q, 3, THR, FRAC, smooth_mode=mode)
    cp = s["corr_positive"]
    assert cp.max() == 128000000.0 and np.array_equal(np.flatnonzero(cp == cp.max()), np.arange(291, 700))
    ev, segs, _ = O.detect_minn_rtl(cp, s["above_threshold"], s["metric_valid"], 2, 0)
    assert ev.tolist() == [[699, 699, 193, 830]] and segs.tolist() == [[193, 830], [891, 1200]]
    iq = np.zeros((1, 1, T, 2), np.int16)
    iq[0, 0, :, 0] = x.real
    ref = _Ref(iq, Q, par)
    assert ref.events[0].tolist() == [[699, 699, 193, 830]] and int(ref.open[0]) == 891
    assert sum(chunks) == T and sum(chunks[:2]) == 700 and sum(chunks[:3]) == 830
    det = _detector(1, 1, Q, par)
    res = _feed(det, _pieces(iq, chunks), final=True)
    torch.cuda.synchronize()
    assert [int(r.open_gate_start[0]) for r in res] == [193, 193, -1, 891]
    assert [int(r.n_events[0]) for r in res] == [0, 0, 1, 0]
    assert res[2].events[0, 0].tolist() == [699, 699, 193, 830]
    _assert_equal(res, ref)
    _assert_oracle(res, iq, Q, par, (0,))


def test_carried_state_below_the_fma_guard():
    """4. shift 1 over a long all-zero tail: the float state halves per sample down into the
    subnormals.  Edges: (a) where the valid state is still exactly 0 (before the burst), (b) right
    after a sample whose state is non-zero and below 2^-700 - the segment that follows is interior and
    must NOT take the fma path, (c) where the state has reached 2^-1074.  With c = 0 the reference's
    s + (0 - s) / 2 never returns to exactly 0: s / 2 is exact while normal, and at s = 2^-1074 the
    quotient -2^-1075 rounds to -0 (ties to even), so 2^-1074 is a fixed point; edge (c) sits on it,
    and the exactly-0 carried state is the one of edge (a)."""
    Q, T, B, hyst = 64, 2600, 2, 2
    par = _par("float", 1, hyst)
    rng = np.random.default_rng(4)
    a = np.round(rng.normal(0, 500, Q) + 1j * rng.normal(0, 500, Q))
    x = np.zeros((B, T), np.complex128)
    x[0, 600:600 + 4 * Q] = np.concatenate([a, a, -a, -a])
    x[1, 563:563 + 4 * Q] = np.concatenate([a, a, -a, -a])     # 37 samples ahead: 2^-37 of stream 0's state
    assert T - (600 + 4 * Q) >= 1500
    iq = np.stack([x.real, x.imag], -1).astype(np.int16)[:, None]
    sm = [O.minn_rtl_metric(x[b], Q, 1, THR, FRAC)["smooth_metric"] for b in range(B)]
    e0 = 450
    e1 = int(np.flatnonzero((sm[0] > 0) & (sm[0] < 2.0 ** -700))[0]) + 1
    e2 = int(np.flatnonzero(sm[0] == 2.0 ** -1074)[0]) + 1
    for b in range(B):
        assert sm[b][e0 - 1] == 0.0 and e0 - 1 >= 3 * Q - 1            # valid and exactly 0
        assert 0.0 < sm[b][e1 - 1] < 2.0 ** -700, sm[b][e1 - 1]        # carried below the guard
    assert sm[0][e2 - 1] == 2.0 ** -1074 and sm[0][-1] == 2.0 ** -1074   # the fixed point, held to the end
    assert e2 - e1 >= 256 and T - e2 >= 256                              # an interior segment follows each edge
    ref = _Ref(iq, Q, par)
    _both_passes(iq, ref, Q, par, [e0, e1 - e0, e2 - e1, T - e2], oracle=(0, 1))


def test_past_the_one_shot_limit():
    """5. T * n_br > 2^21: no one-shot integer-exact plan; float mode against the C oracle.  Bursts
    before and after sample 2^20, two of them over a chunk edge; unequal chunks up to max_chunk."""
    B, nb, Q, hyst = 2, 2, 64, 2
    T = (1 << 20) + 5000
    assert T * nb > 1 << 21 and _lib.lib().ofs_rtl_plan(_lib.CI16, nb, T, Q) == 0
    par = _par("float", 3, hyst)
    det = _detector(B, nb, Q, par)
    assert det.max_chunk == (1 << 20) - 3 * Q
    chunks = [3000, det.max_chunk, T - 3000 - det.max_chunk]
    assert min(chunks) >= 1 and 3000 + det.max_chunk > 1 << 20
    rng = np.random.default_rng(5)
    iq = np.clip(np.round(rng.normal(0, 60, (B, nb, T, 2))), -2048, 2047).astype(np.int16)
    a = np.round(rng.normal(0, 500, Q) + 1j * rng.normal(0, 500, Q))
    burst = np.concatenate([a, a, -a, -a])
    edge2 = 3000 + det.max_chunk
    for s0 in (2900, 600000, edge2 - 100):                     # over edge 3000, mid-stream, over edge2 > 2^20
        iq[0, :, s0:s0 + 4 * Q, 0] = np.clip(iq[0, :, s0:s0 + 4 * Q, 0] + burst.real, -2048, 2047)
        iq[0, :, s0:s0 + 4 * Q, 1] = np.clip(iq[0, :, s0:s0 + 4 * Q, 1] + burst.imag, -2048, 2047)
    xt = torch.from_numpy(iq).cuda()
    res, s = [], 0
    for i, c in enumerate(chunks):
        res.append(_snap(det.push(xt[:, :, s:s + c], final=i == len(chunks) - 1)))
        s += c
    torch.cuda.synchronize()
    want = oracle_c.minn_rtl(iq[..., 0].astype(np.float64) + 1j * iq[..., 1], Q, smooth_shift=3, threshold_value=THR,
                             threshold_frac_bits=FRAC, hysteresis=hyst, timing_offset=TOFF, max_events=1024)
    assert want["n_events"].max() <= 1024
    for k in KEYS:
        got = torch.cat([getattr(r, k) for r in res], dim=1).cpu().numpy()
        assert np.array_equal(got, want[k].astype(got.dtype)), k
    peaks = []
    for b in range(B):
        n = [int(r.n_events[b]) for r in res]
        assert max(n) <= MAX_EV, n
        ev = np.concatenate([r.events[b, :k].cpu().numpy() for r, k in zip(res, n)])
        assert np.array_equal(ev, want["events"][b, :want["n_events"][b]]), b
        assert int(res[-1].open_gate_start[b]) == int(want["open_gate_start"][b])
        peaks += ev[:, 0].tolist()
    near = [p for s0 in (2900, 600000, edge2 - 100) for p in peaks if s0 <= p <= s0 + 6 * Q]
    assert len(near) >= 3 and max(peaks) > 1 << 20, peaks
    with pytest.raises(ValueError, match=str(det.max_chunk)):
        det.push(torch.zeros((B, nb, det.max_chunk + 1, 2), dtype=torch.int16, device="cuda"))


def _three_bursts():
    Q, T = 64, 4000
    rng = np.random.default_rng(7)
    x = rng.normal(0, 60, (2, 1, T)) + 1j * rng.normal(0, 60, (2, 1, T))
    for s0 in (400, 1300, 2200):
        a = rng.normal(0, 500, Q) + 1j * rng.normal(0, 500, Q)
        x[0, 0, s0:s0 + 4 * Q] += np.concatenate([a, a, -a, -a])
    iq = np.stack([np.clip(np.round(x.real), -2048, 2047), np.clip(np.round(x.imag), -2048, 2047)], -1).astype(np.int16)
    return Q, T, iq


def test_event_overflow_keeps_exact_count():
    """6a. max_events = 1 with at least 3 gates closing in one chunk: the count is the true one, only
    slot 0 is written, and the next chunk's results are still exact."""
    Q, T, iq = _three_bursts()
    par = _par("float", 3, 2)
    ref = _Ref(iq, Q, par)
    cut = 3000
    first = [e for e in ref.events[0].tolist() if e[3] <= cut]
    later = [e for e in ref.events[0].tolist() if e[3] > cut]
    assert len(first) >= 3
    det = _detector(2, 1, Q, par, max_events=1)
    res = _feed(det, _pieces(iq, [cut, T - cut]), final=True)
    # the C ABI with room for 4 events but max_events = 1: slots 1.. keep their sentinel
    st = torch.zeros((1, int(_lib.lib().ofs_rtl_chunk_state_bytes(1, Q))), dtype=torch.uint8, device="cuda")
    x0 = torch.tensor(np.ascontiguousarray(iq[:1, :, :cut])).cuda()
    ev = torch.full((1, 4, 4), -7, dtype=torch.int64, device="cuda")
    n_ev = torch.zeros((1,), dtype=torch.int32, device="cuda")
    og = torch.zeros((1,), dtype=torch.int64, device="cuda")
    rc = _lib.lib().ofs_minn_rtl_chunk(_lib.CI16, x0.data_ptr(), 1, 1, cut, Q, 3, 0, THR, FRAC, st.data_ptr(),
                                       None, None, None, None, None, None, None, None, 1, 2, TOFF, 1,
                                       n_ev.data_ptr(), ev.data_ptr(), og.data_ptr(), 0, _lib.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert int(res[0].n_events[0]) == len(first) and res[0].events[0, 0].tolist() == first[0]
    assert int(res[1].n_events[0]) == len(later) and (not later or res[1].events[0, 0].tolist() == later[0])
    for k in KEYS:
        assert torch.equal(torch.cat([getattr(r, k) for r in res], dim=1), getattr(ref.r, k)), k
    assert torch.equal(res[-1].open_gate_start, ref.open)
    assert int(n_ev[0]) == len(first) and ev[0, 0].tolist() == first[0]
    assert bool((ev[0, 1:] == -7).all())


def test_per_stream_reset_mid_gate():
    """6b. reset(mask) inside an open gate of stream 0: the reset streams continue as a fresh detector
    fed the remainder (indices from 0, the open gate forgotten), the others are unaffected."""
    Q, T, iq = _three_bursts()
    iq = np.concatenate([iq, iq[:, :, ::-1]], axis=0)          # B = 4: streams 2, 3 = 0, 1 reversed in time
    iq = np.ascontiguousarray(iq)
    par = _par("float", 3, 40)
    ref = _Ref(iq, Q, par)
    peak, _, start, end = ref.events[0][0].tolist()
    cut = (start + end) // 2
    assert start < cut < end - 1
    tail = _Ref(np.ascontiguousarray(iq[:, :, cut:]), Q, par)
    det = _detector(4, 1, Q, par)
    pieces = _pieces(iq, [cut, 700, T - cut - 700])
    res = _feed(det, pieces[:1], final=False)
    det.reset(torch.tensor([True, True, False, False]))
    res += _feed(det, pieces[1:], final=True)
    torch.cuda.synchronize()
    assert int(res[0].open_gate_start[0]) == start             # the gate was open when the stream was reset
    _assert_equal(res, ref, streams=(2, 3), what="kept")
    _assert_equal(res[1:], tail, streams=(0, 1), what="reset")
    det.reset()
    assert det.samples_seen == 0 and not bool(det.state.any())


def test_chunks_enqueued_without_host_synchronisation():
    """7. All chunks of the first split shape enqueued back to back (inputs uploaded beforehand, each
    result cloned on the same stream), one synchronisation at the end; an events-only detector runs
    with every array output null."""
    B, nb, T, Q, hyst, chunks = SPLITS[0]
    seed = B * 7 + Q
    iq, ref = _stream(seed, B, nb, T, Q), _ref(seed, B, nb, T, Q, "float", 3, hyst)
    pieces = _pieces(iq, chunks)
    det = _detector(B, nb, Q, _par("float", 3, hyst))
    only = _detector(B, nb, Q, _par("float", 3, hyst), outputs=())
    torch.cuda.synchronize()
    res, res_only = [], []
    for i, p in enumerate(pieces):                             # nothing below waits for the GPU
        res.append(_snap(det.push(p, final=i == len(pieces) - 1)))
        res_only.append(_snap(only.push(p, final=i == len(pieces) - 1)))
    torch.cuda.synchronize()
    _assert_equal(res, ref, what="back to back")
    for r in res_only:
        assert all(getattr(r, k) is None for k in KEYS)
    for b in range(B):
        ev, n = _events(res_only, b)
        assert n == ref.n[b] and torch.equal(ev, ref.events[b])
    assert torch.equal(res_only[-1].open_gate_start, ref.open)
