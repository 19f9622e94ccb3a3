"""GPU: the resumable zc_v2 CFAR + gate (ofs_zc_detect_chunk, zc_v2.ZCChunkedDetector).

Expected values come from ofdm_oracle on the whole stream (cut per call by arithmetic on its events), from
the NumPy model of tests/zc_chunk_model.py, or from the one-shot ofs_zc_detect - never from the chunk
kernel.  Every output buffer is filled with canaries first.  One rule everywhere: the concatenated arrays
and events EQUAL the one-shot result; a call reports exactly the gates whose closing sample it holds (the
end-of-stream close belongs to the final call), from slot 0, and leaves the slots at or beyond
min(n_events, max_events) untouched; open_gate_start is the start of the gate that spans the call's end;
and gate_mask differs from the one-shot mask in no sample, or in exactly the start sample of a gate that
the final call closed when that sample lies in an earlier call.
"""
import numpy as np
import pytest
import torch

import zc_chunk_model as M
import zc_gate_streams as Z
from ofdm_sync_amd import _lib, zc_v2

pytestmark = pytest.mark.gpu

E = 16
CAN_I, CAN_F, CAN_U8, CAN_N = -77, -77.0, 0xA5, -5
F64 = ("local_sum", "corr_scaled", "thresh_scaled")
U8 = ("above_threshold", "metric_valid")
SHAPES = ((1024, 128), (1152, 256), (2304, 1024), (1000, 128), (1024, 100), (130, 128), (64, 32))


def hysts(n):
    return (0, 1, 2, 63, 64, 65, 127, 128, 129, 256, n + 7)


def new_state(B, W):
    nb = int(_lib.lib().ofs_zc_chunk_state_bytes(int(W)))
    assert nb > 0
    return torch.zeros((B, nb), dtype=torch.uint8, device="cuda")


class Run:
    """The calls of one batch under one split, launched back to back on canary-filled buffers (one
    synchronisation at the end).  chunks: one [B, Tc] device tensor per call, passed in place with its
    row stride (Tc = 0: a flush).  finals[k]: the call's `final`."""

    def __init__(self, chunks, finals, params, hyst, state_arrays, max_ev=E, reflen=Z.REFLEN, st=None,
                 null_events=False):
        W, tv, f, mn = params
        B = chunks[0].shape[0]
        K = len(chunks)
        lens = [int(c.shape[1]) for c in chunks]
        n = sum(lens)
        dev = "cuda"
        self.st = new_state(B, W) if st is None else st
        names = (F64 + U8 if state_arrays else ()) + ("gate_mask",)
        flat = {k: torch.full((B * n,), CAN_F if k in F64 else CAN_U8,
                              dtype=torch.float64 if k in F64 else torch.uint8, device=dev) for k in names}
        EE = max(max_ev, 1)
        n_ev = torch.full((K, B), CAN_N, dtype=torch.int32, device=dev)
        ev_i = torch.full((K, B, EE, 4), CAN_I, dtype=torch.int64, device=dev)
        ev_v = torch.full((K, B, EE), CAN_F, dtype=torch.float64, device=dev)
        op = torch.full((K, B), CAN_I, dtype=torch.int64, device=dev)
        fn = _lib.lib().ofs_zc_detect_chunk
        at = 0
        for k, (c, fin) in enumerate(zip(chunks, finals)):
            Tc = lens[k]
            assert c.dtype == torch.float64 and (Tc == 0 or c.stride(1) == 1)
            p = lambda key: flat[key][B * at:].data_ptr() if key in flat and Tc else None  # noqa: E731
            rc = fn(c.data_ptr() if Tc else None, c.stride(0) if Tc and B > 1 else Tc, B, Tc, int(W), int(tv), int(f),
                    float(mn), int(reflen), int(hyst), self.st.data_ptr(), p("local_sum"), p("corr_scaled"),
                    p("thresh_scaled"), p("above_threshold"), p("metric_valid"), p("gate_mask"), max_ev,
                    n_ev[k].data_ptr(), None if null_events else ev_i[k].data_ptr(),
                    None if null_events else ev_v[k].data_ptr(), op[k].data_ptr(), int(fin),
                    torch.cuda.current_stream().cuda_stream)
            assert rc == 0, (rc, k, Tc)
            at += Tc
        torch.cuda.synchronize()
        self.B, self.n, self.K, self.lens, self.max_ev = B, n, K, lens, max_ev
        self.arr = {}
        for key, t in flat.items():
            h, parts, at = t.cpu().numpy(), [], 0
            for Tc in lens:
                parts.append(h[B * at:B * (at + Tc)].reshape(B, Tc))
                at += Tc
            self.arr[key] = np.concatenate(parts, axis=1)
        self.n_ev, self.ev_i, self.ev_v, self.op = (x.cpu().numpy() for x in (n_ev, ev_i, ev_v, op))

    def all_events(self, b):
        """The stream's events of every call in order (only what the slots hold)."""
        rows, vals = [], []
        for k in range(self.K):
            m = min(int(self.n_ev[k, b]), self.max_ev)
            rows.append(self.ev_i[k, b, :m])
            vals.append(self.ev_v[k, b, :m])
        return np.concatenate(rows).reshape(-1, 4), np.concatenate(vals)


def expect_calls(ev, vals, ends, n_total, max_ev):
    """Per-call expectations of one stream from its whole-stream events (gate_end sorted, the end close at
    n_total): (n_events [K], events [K, EE, 4] and peaks [K, EE] with canaries, open_gate_start [K])."""
    K, EE = len(ends), max(max_ev, 1)
    ends = np.asarray(ends, np.int64)
    gs, ge = ev[:, 1], ev[:, 2]
    call = np.searchsorted(ends, ge, side="right")            # first call whose end lies beyond gate_end
    call[ge == n_total] = K - 1                                # closed by `final`
    cnt = np.bincount(call, minlength=K)[:K]
    first = np.searchsorted(call, np.arange(K), side="left")
    slot = np.arange(len(ev)) - first[call] if len(ev) else np.zeros(0, np.int64)
    ei = np.full((K, EE, 4), CAN_I, np.int64)
    pv = np.full((K, EE), CAN_F, np.float64)
    keep = slot < max_ev
    ei[call[keep], slot[keep]] = ev[keep]
    pv[call[keep], slot[keep]] = vals[keep]
    idx = np.searchsorted(gs, ends, side="left") - 1          # the last gate that started before the call's end
    opn = np.where((idx >= 0) & (ge[np.maximum(idx, 0)] >= ends), gs[np.maximum(idx, 0)], -1) \
        if len(ev) else np.full(K, -1)
    return cnt, ei, pv, opn


def check_run(r, exp, order, state_arrays, tag, final_start=None):
    """r: a Run whose last call is final; exp[b]: the whole-stream expectation of the stream in row j =
    order.index(b) (the oracle's dict, or the one-shot call's in the same form).  final_start: first sample of
    the final call (default: where the last call starts)."""
    ends = np.cumsum(r.lens)
    fs = int(ends[-1] - r.lens[-1]) if final_start is None else final_start
    for j, b in enumerate(order):
        e, t = exp[b], (tag, j, b)
        cnt, ei, pv, opn = expect_calls(e["events"], e["peak_values"], ends, r.n, r.max_ev)
        assert np.array_equal(r.n_ev[:, j], cnt), (t, r.n_ev[:, j].tolist(), cnt.tolist())
        assert int(r.n_ev[:, j].sum()) == len(e["events"]), t
        assert np.array_equal(r.op[:, j], opn), (t, r.op[:, j].tolist(), opn.tolist())
        assert np.array_equal(r.ev_i[:, j], ei), (t, r.ev_i[:, j].tolist(), ei.tolist())
        assert np.array_equal(r.ev_v[:, j], pv), t
        mask = e["gate_mask"].astype(np.uint8).copy()
        if opn[-1] >= 0 and opn[-1] < fs:
            assert mask[opn[-1]] == 1
            mask[opn[-1]] = 0                                   # the one mask exception
        assert np.array_equal(r.arr["gate_mask"][j], mask), (t, np.flatnonzero(r.arr["gate_mask"][j] != mask)[:8])
        if state_arrays:
            for key in F64:
                assert np.array_equal(r.arr[key][j], e[key]), (t, key)
            for key in U8:
                assert np.array_equal(r.arr[key][j], e[key].astype(np.uint8)), (t, key)


def cut(mag, split):
    """Column slices of mag [B, n] (in place: row stride n, any 8-byte alignment)."""
    out, at = [], 0
    for t in split:
        out.append(mag[:, at:at + t])
        at += t
    return out


def finals(split):
    return [False] * (len(split) - 1) + [True]


# ---------------------------------------------------------------------------------------------------
# exact streams against the oracle
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,W", SHAPES, ids=str)
def test_exact_streams_every_split_both_modes(n, W):
    for hyst in hysts(n):
        st, exp = Z.streams(n, W, hyst), Z.expected(n, W, hyst)
        for fam, bt in st.items():
            mag = torch.from_numpy(np.array(bt.c, np.float64)).cuda()
            order = range(len(bt.names))
            for k, split in enumerate(M.splits(n, W, 31 * n + hyst)):
                for state_arrays in (True, False):
                    r = Run(cut(mag, split), finals(split), bt.params, hyst, state_arrays)
                    check_run(r, exp[fam], order, state_arrays, (n, W, hyst, fam, k, state_arrays))


def test_both_mask_outcomes_occur():
    """The exception sample and the exception-free case both occur among the checked streams (the model
    test asserts the same on the CPU; here on the kernel's outputs)."""
    n, W, hyst = 1000, 128, 256
    bt, exp = Z.streams(n, W, hyst)["M"], Z.expected(n, W, hyst)["M"]
    mag = torch.from_numpy(np.array(bt.c, np.float64)).cuda()
    split = [333, 333, 334]
    r = Run(cut(mag, split), finals(split), bt.params, hyst, False)
    check_run(r, exp, range(len(bt.names)), False, "outcomes")
    differs = [int((r.arr["gate_mask"][b] != exp[b]["gate_mask"]).sum()) for b in range(len(bt.names))]
    assert set(differs) == {0, 1}


# ---------------------------------------------------------------------------------------------------
# inexact data against the one-shot call
# ---------------------------------------------------------------------------------------------------
def one_shot(mag, params, hyst, reflen=Z.REFLEN, max_ev=64):
    """ofs_zc_detect on mag [B, n] (contiguous), as a list of per-stream dicts in the oracle's form."""
    B, n = mag.shape
    W, tv, f, mn = params
    out = {k: torch.full((B, n), CAN_F if k in F64 else CAN_U8, dtype=torch.float64 if k in F64 else torch.uint8,
                         device="cuda") for k in F64 + U8 + ("gate_mask",)}
    n_ev = torch.full((B,), CAN_N, dtype=torch.int32, device="cuda")
    ev_i = torch.full((B, max_ev, 4), CAN_I, dtype=torch.int64, device="cuda")
    ev_v = torch.full((B, max_ev), CAN_F, dtype=torch.float64, device="cuda")
    rc = _lib.lib().ofs_zc_detect(mag.data_ptr(), B, n, int(W), int(tv), int(f), float(mn), int(reflen), int(hyst),
                                  *(out[k].data_ptr() for k in F64 + U8 + ("gate_mask",)), max_ev,
                                  n_ev.data_ptr(), ev_i.data_ptr(), ev_v.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    cnt, ei, ev = n_ev.cpu().numpy(), ev_i.cpu().numpy(), ev_v.cpu().numpy()
    assert cnt.max() <= max_ev
    return [dict({k: h[k][b] for k in h}, events=ei[b, :cnt[b]], peak_values=ev[b, :cnt[b]]) for b in range(B)]


def random_mag(B, n, seed):
    rng = np.random.default_rng(seed)
    c = np.abs(rng.standard_normal((B, n)))
    for b in range(0, B, 2):                                   # pulses of 5-20 in every other stream
        for p in rng.choice(np.arange(150, n - 5), size=6, replace=False):
            c[b, p:p + int(rng.integers(1, 4))] = rng.uniform(5.0, 20.0)
    return c


@pytest.mark.parametrize("W", [100, 128])
@pytest.mark.parametrize("hyst", [3, 256])
def test_bit_for_bit_against_one_shot_on_inexact_data(W, hyst):
    n = 2000
    params = (W, int(4.0 * (1 << 15) / W), 15, 0.3)
    rng = np.random.default_rng(W + hyst)
    cuts = np.sort(rng.choice(np.arange(1, n), size=5, replace=False))
    split_list = ([700, 700, 600], [129] * 15 + [65], np.diff(np.concatenate(([0], cuts, [n]))).astype(int).tolist())
    for B in (1, 15, 16, 17, 33):
        c = random_mag(B, n, 7 * B + W)
        assert not np.array_equal(c * 16.0, np.round(c * 16.0))
        mag = torch.from_numpy(c).cuda()
        ref = one_shot(mag, params, hyst)
        for b in range(0, B, 2):
            assert len(ref[b]["events"]) >= 1, (B, b)
        for split in split_list:
            for state_arrays in (True, False):
                r = Run(cut(mag, split), finals(split), params, hyst, state_arrays, max_ev=64)
                check_run(r, ref, range(B), state_arrays, (W, hyst, B, split[:3], state_arrays))


# ---------------------------------------------------------------------------------------------------
# streams at different n in one call
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyst", [3, 256])
def test_partial_reset_puts_streams_at_different_n(hyst):
    """After two pushes the state rows of every third stream are zeroed: those streams go on as the
    sub-stream that starts at the reset, the others as the whole stream (per-stream fill phase)."""
    n, W, B = 1200, 128, 20
    params = (W, int(4.0 * (1 << 15) / W), 15, 0.3)
    c = random_mag(B, n, 99)
    mag = torch.from_numpy(c).cuda()
    split = [200, 150, 100, 350, 400]
    t_reset = 350
    st = new_state(B, W)
    a = Run(cut(mag, split)[:2], [False, False], params, hyst, True, max_ev=64, st=st)
    st[::3].zero_()
    b = Run(cut(mag, split)[2:], [False, False, True], params, hyst, True, max_ev=64, st=st)
    ends_b = np.cumsum(split[2:])
    for s in range(B):                                              # the two calls before the reset
        e = Z.run_oracle(c[s], params, hyst)
        cnt, ei, pv, opn = expect_calls(e["events"], e["peak_values"], np.cumsum(split), n, 64)
        assert np.array_equal(a.n_ev[:, s], cnt[:2]) and np.array_equal(a.op[:, s], opn[:2]), s
        assert np.array_equal(a.ev_i[:, s], ei[:2]) and np.array_equal(a.ev_v[:, s], pv[:2]), s
        for key in F64:
            assert np.array_equal(a.arr[key][s], e[key][:t_reset]), (s, key)
        for key in U8:
            assert np.array_equal(a.arr[key][s], e[key][:t_reset].astype(np.uint8)), (s, key)
        # before the final call no start sample is ever set: the mask is the one-shot mask except that sample
        mask = e["gate_mask"][:t_reset].astype(np.uint8).copy()
        if len(e["events"]) and e["events"][-1, 2] == n and e["events"][-1, 1] < t_reset:
            mask[e["events"][-1, 1]] = 0
        assert np.array_equal(a.arr["gate_mask"][s], mask), s
    for s in range(B):
        if s % 3 == 0:                                          # a fresh stream from t_reset on
            e = Z.run_oracle(c[s, t_reset:], params, hyst)
            cnt, ei, pv, opn = expect_calls(e["events"], e["peak_values"], ends_b, n - t_reset, 64)
            for key in F64:
                assert np.array_equal(b.arr[key][s], e[key]), (s, key)
            for key in U8:
                assert np.array_equal(b.arr[key][s], e[key].astype(np.uint8)), (s, key)
            mask = e["gate_mask"].astype(np.uint8).copy()
            if opn[-1] >= 0 and opn[-1] < ends_b[-1] - split[-1]:
                mask[opn[-1]] = 0
            assert np.array_equal(b.arr["gate_mask"][s], mask), s
        else:
            e = Z.run_oracle(c[s], params, hyst)
            ends = np.cumsum(split)
            cnt, ei, pv, opn = expect_calls(e["events"], e["peak_values"], ends, n, 64)
            cnt, ei, pv, opn = cnt[2:], ei[2:], pv[2:], opn[2:]
            for key in F64:
                assert np.array_equal(np.concatenate((a.arr[key][s], b.arr[key][s])), e[key]), (s, key)
            for key in U8:
                assert np.array_equal(np.concatenate((a.arr[key][s], b.arr[key][s])), e[key].astype(np.uint8)), (s, key)
            mask = e["gate_mask"].astype(np.uint8).copy()
            if opn[-1] >= 0 and opn[-1] < n - split[-1]:
                mask[opn[-1]] = 0
            assert np.array_equal(np.concatenate((a.arr["gate_mask"][s], b.arr["gate_mask"][s])), mask), s
        assert np.array_equal(b.n_ev[:, s], cnt), (s, b.n_ev[:, s], cnt)
        assert np.array_equal(b.ev_i[:, s], ei) and np.array_equal(b.ev_v[:, s], pv), s
        assert np.array_equal(b.op[:, s], opn), s


# ---------------------------------------------------------------------------------------------------
# strided, misaligned input
# ---------------------------------------------------------------------------------------------------
def test_strided_misaligned_input_equals_dense():
    n, W, hyst = 1000, 128, 64
    bt, exp = Z.streams(n, W, hyst)["M"], Z.expected(n, W, hyst)["M"]
    c = np.array(bt.c, np.float64)
    B = c.shape[0]
    split = [333, 300, 367]
    dense, wide, at = [], [], 0
    for t in split:
        d = torch.from_numpy(c[:, at:at + t].copy()).cuda()
        w = torch.full((B, t + 5), 1e9, dtype=torch.float64, device="cuda")
        w[:, 1:1 + t] = d
        v = w[:, 1:1 + t]
        assert d.is_contiguous() and v.stride(0) == t + 5 and v.data_ptr() % 16 == 8
        dense.append(d)
        wide.append(v)
        at += t
    a = Run(dense, finals(split), bt.params, hyst, True)
    b = Run(wide, finals(split), bt.params, hyst, True)
    check_run(a, exp, range(B), True, "dense")
    check_run(b, exp, range(B), True, "strided")
    for key in a.arr:
        assert np.array_equal(a.arr[key], b.arr[key]), key
    assert np.array_equal(a.ev_i, b.ev_i) and np.array_equal(a.ev_v, b.ev_v) and np.array_equal(a.n_ev, b.n_ev)


# ---------------------------------------------------------------------------------------------------
# overflow, events off
# ---------------------------------------------------------------------------------------------------
def test_event_overflow_and_events_off():
    n, W, hyst = 1024, 128, 64
    bt, exp = Z.streams(n, W, hyst)["M"], Z.expected(n, W, hyst)["M"]
    assert max(len(e["events"]) for e in exp) > 8
    mag = torch.from_numpy(np.array(bt.c, np.float64)).cuda()
    order = range(len(bt.names))
    for split in ([n], [512, 512]):
        r = Run(cut(mag, split), finals(split), bt.params, hyst, False, max_ev=2)
        assert r.n_ev.max() > 2
        check_run(r, exp, order, False, ("overflow", split))           # exact counts, canaries past slot 2
        z = Run(cut(mag, split), finals(split), bt.params, hyst, False, max_ev=0, null_events=True)
        check_run(z, exp, order, False, ("events off", split))         # counts, mask and open_gate_start only


# ---------------------------------------------------------------------------------------------------
# final against flush; the state afterwards
# ---------------------------------------------------------------------------------------------------
def test_final_equals_flush_and_leaves_fresh_streams():
    n, W, hyst = 1000, 128, 256
    bt, exp = Z.streams(n, W, hyst)["M"], Z.expected(n, W, hyst)["M"]
    B = len(bt.names)
    mag = torch.from_numpy(np.array(bt.c, np.float64)).cuda()
    split = [400, 600]
    sa, sb = new_state(B, W), new_state(B, W)
    a = Run(cut(mag, split), [False, True], bt.params, hyst, True, st=sa)
    empty = torch.empty((B, 0), dtype=torch.float64, device="cuda")
    b = Run(cut(mag, split) + [empty], [False, False, True], bt.params, hyst, True, st=sb)
    check_run(a, exp, range(B), True, "final")
    # the flush: the same events one call later, no mask store at all (every open gate's start is earlier)
    check_run(b, exp, range(B), True, "flush", final_start=n)
    assert int(b.n_ev[2].sum()) > 0 and np.array_equal(a.n_ev[1], b.n_ev[1] + b.n_ev[2])
    for j in range(B):
        ea, va = a.all_events(j)
        eb, vb = b.all_events(j)
        assert np.array_equal(ea, eb) and np.array_equal(va, vb), j
    assert np.array_equal(a.op[1], b.op[2]) and np.array_equal(b.op[1], b.op[2])
    assert not sa.any().item() and not sb.any().item()                # fresh = all-zero bytes
    # a second, different stream through the used rows equals a new zero state
    other = torch.from_numpy(np.array(bt.c[::-1], np.float64)).cuda()
    rev = list(range(B))[::-1]
    for st in (sa, sb, None):
        r = Run(cut(other, [300, 700]), [False, True], bt.params, hyst, True, st=st)
        check_run(r, exp, rev, True, "second stream")


def test_single_samples_and_tiny_windows():
    """Tc = 1 calls throughout a short stream, W = 1 (window_size 0 and 1) and hysteresis 0."""
    rng = np.random.default_rng(5)
    n, B = 70, 9
    c = np.round(rng.uniform(0, 4, (B, n)) * 16) / 16
    mag = torch.from_numpy(c).cuda()
    for ws in (0, 1, 3):
        params = (ws, 1 << 14, 15, 0.5)
        exp = [Z.run_oracle(c[b], params, 0) for b in range(B)]
        assert sum(len(e["events"]) for e in exp) > B
        split = [1] * n
        r = Run(cut(mag, split), finals(split), params, 0, True, max_ev=4)
        check_run(r, exp, range(B), True, ("tiny", ws))


# ---------------------------------------------------------------------------------------------------
# product level: ZCChunkedDetector against detect_zc_preamble_batched
# ---------------------------------------------------------------------------------------------------
def zc_ref(N=100):
    k = np.arange(N)
    return np.exp(-1j * np.pi * 25 * k * (k + 1) / N)


def planted(B, nb, T, ref, plants, seed, sigma=0.05):
    rng = np.random.default_rng(seed)
    x = sigma * (rng.standard_normal((B, nb, T)) + 1j * rng.standard_normal((B, nb, T)))
    for b in range(0, B, 2):
        for p in plants:
            x[b, :, p:p + len(ref)] += ref[:T - p]
    return x


def as_input(x, kind):
    if kind == "complex128":
        return torch.from_numpy(x).cuda()
    if kind == "complex64":
        return torch.from_numpy(x.astype(np.complex64)).cuda()
    q = np.stack((np.round(x.real * 2048), np.round(x.imag * 2048)), axis=-1).astype(np.int16)
    return torch.from_numpy(q).cuda()


def run_product(xd, ref, split, nb, normalize, hyst, W, tv, method="auto", max_events=8):
    """(one-shot result, concatenated chunked results) for one input."""
    B, T = xd.shape[0], xd.shape[2]
    one = zc_v2.detect_zc_preamble_batched(xd, ref, W, tv, 15, 0.3, hyst, normalize, max_events=max_events,
                                           want_state=False, method=method)
    det = zc_v2.ZCChunkedDetector(B, ref, nb, window_size=W, thresh_value=tv, thresh_frac_bits=15,
                                  min_corr_mag=0.3, hysteresis=hyst, normalize=normalize, max_events=max_events)
    mags, masks, evs, pvs, at = [], [], [[] for _ in range(B)], [[] for _ in range(B)], 0

    def take(r):
        mags.append(r.corr_mag.clone())
        masks.append(r.gate_mask.clone())
        cnt = r.n_events.cpu().numpy()
        assert cnt.max() <= max_events
        for b in range(B):
            evs[b].append(r.events[b, :cnt[b]].cpu().numpy())
            pvs[b].append(r.peak_values[b, :cnt[b]].cpu().numpy())
        return r

    for k, t in enumerate(split):
        piece = xd[:, :, at:at + t]
        at += t
        r = take(det.push(piece, final=(k == len(split) - 1)))
        assert (r.tail is not None) == (k == len(split) - 1)
    last = take(r.tail)
    assert not det.state.any().item() and det.history is None
    return one, torch.cat(mags, dim=1), torch.cat(masks, dim=1), evs, pvs, last


@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("normalize", [True, False])
def test_product_level_equals_one_shot(nb, normalize):
    ref = zc_ref(100)
    B, T, W, N = 6, 1500, 128, 100
    tv = int(4 * 2 ** 15 / 128)
    x = planted(B, nb, T, ref, (300, 900), 11 + nb)
    rng = np.random.default_rng(3)
    cuts = np.sort(rng.choice(np.arange(1, T), size=4, replace=False))
    split_list = ([T], [256] * 5 + [220], np.diff(np.concatenate(([0], cuts, [T]))).astype(int).tolist())
    for kind in ("complex128", "complex64", "int16"):
        xd = as_input(x, kind)
        for split in split_list:
            one, mag, mask, evs, pvs, last = run_product(xd, ref, split, nb, normalize, 64, W, tv)
            assert mag.shape == (B, T + N - 1) and torch.equal(mag, one.corr_mag), (kind, split[:3])
            cnt = one.n_events.cpu().numpy()
            for b in range(B):
                if normalize:                                       # the counts the issue states, one-shot side
                    assert cnt[b] == (2 if b % 2 == 0 else 0), (kind, b, cnt[b])
                    if b % 2 == 0:
                        assert one.events[b, :2, 0].tolist() == [399, 999]
                assert np.array_equal(np.concatenate(evs[b]).reshape(-1, 4), one.events[b, :cnt[b]].cpu().numpy()), (kind, b)
                assert np.array_equal(np.concatenate(pvs[b]), one.peak_values[b, :cnt[b]].cpu().numpy()), (kind, b)
            # no gate is open at the end here, so the masks are equal without exception
            assert (last.open_gate_start == -1).all().item()
            assert torch.equal(mask, one.gate_mask), (kind, split[:3])
    if normalize:
        assert cnt[::2].sum() >= 2


@pytest.mark.parametrize("nb", [1, 2])
def test_product_level_gate_closed_by_the_end_of_the_stream(nb):
    """Hysteresis 256 and a plant at 1380: the gate is still open at T + N - 1 = 1599 and flush() closes it
    there, as the one-shot call does."""
    ref = zc_ref(100)
    B, T, W = 6, 1500, 128
    tv = int(4 * 2 ** 15 / 128)
    x = planted(B, nb, T, ref, (300, 1380), 21 + nb)
    xd = as_input(x, "complex128")
    for split in ([T], [256] * 5 + [220], [1400, 100]):
        one, mag, mask, evs, pvs, last = run_product(xd, ref, split, nb, True, 256, W, tv)
        assert torch.equal(mag, one.corr_mag)
        cnt = one.n_events.cpu().numpy()
        for b in range(0, B, 2):
            ev = one.events[b, :cnt[b]].cpu().numpy()
            assert ev[-1, 0] == 1479 and ev[-1, 2] == 1599 and ev[-1, 3] == 1380 and 1380 <= ev[-1, 1] <= 1479, ev
            assert np.array_equal(np.concatenate(evs[b]).reshape(-1, 4), ev), (b, split[:3])
            assert np.array_equal(np.concatenate(pvs[b]), one.peak_values[b, :cnt[b]].cpu().numpy())
            assert int(last.open_gate_start[b]) == ev[-1, 1]
            # the mask differs only in the gate's start sample, which lies before the flush's samples
            d = torch.nonzero(mask[b] != one.gate_mask[b]).flatten().tolist()
            assert d == ([int(ev[-1, 1])] if ev[-1, 1] < T else []), (b, d)
        for b in range(1, B, 2):
            assert cnt[b] == 0 and torch.equal(mask[b], one.gate_mask[b])


def test_product_level_long_reference_direct():
    """A 300-tap reference: the one-shot side must use the direct sums too (method="direct")."""
    ref = zc_ref(300)
    B, T, W = 4, 1500, 128
    tv = int(4 * 2 ** 15 / 128)
    x = planted(B, 1, T, ref, (300, 900), 5)
    xd = as_input(x, "complex128")
    one, mag, mask, evs, pvs, last = run_product(xd, ref, [500, 1000], 1, True, 64, W, tv, method="direct")
    assert mag.shape == (B, T + 299) and torch.equal(mag, one.corr_mag)
    cnt = one.n_events.cpu().numpy()
    assert cnt[::2].min() >= 1
    for b in range(B):
        assert np.array_equal(np.concatenate(evs[b]).reshape(-1, 4), one.events[b, :cnt[b]].cpu().numpy())
        assert np.array_equal(np.concatenate(pvs[b]), one.peak_values[b, :cnt[b]].cpu().numpy())


def test_detector_reset_mask_and_push_mag():
    """push_mag on a column slice, reset(mask) of some streams: they restart as fresh streams."""
    n, W, hyst = 1000, 128, 64
    bt = Z.streams(n, W, hyst)["M"]
    B = len(bt.names)
    Wp, tv, f, mn = bt.params
    mag = torch.from_numpy(np.array(bt.c, np.float64)).cuda()
    det = zc_v2.ZCChunkedDetector(B, np.ones(Z.REFLEN, complex), 1, window_size=Wp, thresh_value=tv, thresh_frac_bits=f,
                                  min_corr_mag=mn, hysteresis=hyst, outputs=("local_sum", "gate_mask"), max_events=E)
    det.push_mag(mag[:, :300])
    m = torch.zeros(B, dtype=torch.bool)
    m[::2] = True
    det.reset(m)
    r = det.push_mag(mag[:, 300:], final=True)
    ls = r.local_sum.cpu().numpy()
    whole = Z.expected(n, W, hyst)["M"]
    for b in range(B):
        e = Z.run_oracle(bt.c[b, 300:], bt.params, hyst) if b % 2 == 0 else whole[b]
        assert np.array_equal(ls[b], e["local_sum"][-700:]), b
    assert not det.state.any().item()


def test_detector_without_event_arrays_and_flush_before_push():
    """max_events=0 reaches the C ABI as 0 with null event arrays (counts, mask and open_gate_start only); a
    flush before any push, or after one, leaves a detector that takes another sample format."""
    n, W, hyst = 1000, 128, 64
    bt, exp = Z.streams(n, W, hyst)["M"], Z.expected(n, W, hyst)["M"]
    B = len(bt.names)
    Wp, tv, f, mn = bt.params
    mag = torch.from_numpy(np.array(bt.c, np.float64)).cuda()
    det = zc_v2.ZCChunkedDetector(B, np.ones(Z.REFLEN, complex), 1, window_size=Wp, thresh_value=tv, thresh_frac_bits=f,
                                  min_corr_mag=mn, hysteresis=hyst, max_events=0)
    assert det.max_events == 0
    r = det.push_mag(mag, final=True)
    r.events.fill_(CAN_I)
    r.peak_values.fill_(CAN_F)
    r = det.push_mag(mag, final=True)
    assert r.n_events.cpu().tolist() == [len(e["events"]) for e in exp] and max(r.n_events.cpu().tolist()) > 8
    assert (r.events == CAN_I).all().item() and (r.peak_values == CAN_F).all().item()
    for b in range(B):
        assert np.array_equal(r.gate_mask[b].cpu().numpy(), exp[b]["gate_mask"].astype(np.uint8)), b
    ref = zc_ref(100)
    T, N, W2, tv2 = 600, 100, 128, int(4 * 2 ** 15 / 128)
    x = planted(2, 1, T, ref, (300,), 4)

    def tail_equals_one_shot(res, xd):
        """The tail of a final push: [B, N - 1] arrays, equal to the one-shot columns T .. T + N - 2."""
        one = zc_v2.detect_zc_preamble_batched(xd, ref, W2, tv2, 15, 0.3, 64, True, want_state=False)
        t = res.tail
        assert t is not None and t.gate_mask is not None and t.corr_mag is not None
        assert tuple(t.gate_mask.shape) == (2, N - 1) == tuple(t.corr_mag.shape)
        assert tuple(res.gate_mask.shape) == (2, T)
        assert (t.open_gate_start == -1).all().item()             # no gate open at the end: no mask exception
        assert torch.equal(torch.cat((res.corr_mag, t.corr_mag), dim=1), one.corr_mag)
        assert torch.equal(torch.cat((res.gate_mask, t.gate_mask), dim=1), one.gate_mask)
        assert int(one.n_events[0]) == 1 == int(res.n_events[0]) + int(t.n_events[0])
        assert int(res.events[0, 0, 0]) == 399 == int(one.events[0, 0, 0])

    det = zc_v2.ZCChunkedDetector(2, ref, 1, window_size=W2, thresh_value=tv2, hysteresis=64)
    t0 = det.flush()                                              # nothing pushed yet: a Tc = 0 call, no arrays
    assert det.history is None and int(t0.n_events.sum()) == 0 and t0.gate_mask is None and t0.corr_mag is None
    xa, xb = as_input(x, "complex64"), as_input(x, "int16")
    a = det.push(xa, final=True)                                  # its tail flush has N - 1 real samples
    assert det.history is None
    tail_equals_one_shot(a, xa)
    t1 = det.flush()                                              # and a Tc = 0 flush after it has none again
    assert t1.gate_mask is None and t1.corr_mag is None and int(t1.n_events.sum()) == 0
    b = det.push(xb, final=True)                                  # another format after the flush
    tail_equals_one_shot(b, xb)
    # push_mag only, then flush: a Tc = 0 final call that closes what push_mag left open; a tail flush after it
    det2 = zc_v2.ZCChunkedDetector(B, np.ones(Z.REFLEN, complex), 1, window_size=Wp, thresh_value=tv, thresh_frac_bits=f,
                                   min_corr_mag=mn, hysteresis=hyst, max_events=E)
    det2.push_mag(mag)
    t2 = det2.flush()
    still_open = [len(e["events"]) > 0 and e["events"][-1, 2] == n for e in exp]
    assert t2.gate_mask is None and t2.n_events.cpu().tolist() == [int(v) for v in still_open] and any(still_open)
    assert not det2.state.any().item()
    det3 = zc_v2.ZCChunkedDetector(2, ref, 1, window_size=W2, thresh_value=tv2, hysteresis=64)
    det3.push_mag(torch.zeros((2, 50), dtype=torch.float64, device="cuda"))
    det3.flush()
    tail_equals_one_shot(det3.push(xa, final=True), xa)
