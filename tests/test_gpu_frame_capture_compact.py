"""GPU: ofs_frame_capture_compact / FrameCapture.push_compact.  The yardstick is a second FrameCapture of
the same parameters fed the same pushes through the slot form: its live() output cut to the first `cap`
rows IS the compact result, bit for bit, after every push, and the two states are equal bytes.  Where
tests/test_gpu_frame_capture.py uses the plain-Python model (tests/capture_model.py), so does this."""
import numpy as np
import pytest
import torch

import capture_model as cm

pytestmark = pytest.mark.gpu

KINDS = {"c64": torch.complex64, "c128": torch.complex128, "i16": torch.int16}
PATTERN = 0x5A                                                    # byte of the pre-filled frame buffer


def raw(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes (same device)."""
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.uint8)


class Pair:
    """A compact capture and its slot-form yardstick, fed alike and compared after every push."""

    def __init__(self, B, n_br, F, H, Q, rows, kind="c64", offset=0):
        from ofdm_sync_amd.capture import FrameCapture
        kw = dict(frame_len=F, history=H, max_pending=Q, offset=offset, dtype=KINDS[kind])
        self.a = FrameCapture(B, n_br, compact_rows=rows, **kw)
        self.b = FrameCapture(B, n_br, **kw)
        self.B, self.rows, self.Q = B, rows, Q
        self.n_rows = []                                          # per push [written, lost]
        self.dropped = torch.zeros((B, 3), dtype=torch.int64)
        self.order = {}                                           # stream -> starts in the order they came out

    def reset(self, mask):
        self.a.reset(mask)
        self.b.reset(mask)

    def push(self, x, starts=None, cnt=None, final=False, flush=False, tag=None, compact=True):
        a, b, rows = self.a, self.b, self.rows
        raw(a._compact.frames).fill_(PATTERN)
        if flush:
            rb = b.flush()
            xa = x[:, :, :0]
            ra = a.push_compact(xa, final=True) if compact else a.flush()
        else:
            rb = b.push(x, starts, cnt, final=final)
            ra = (a.push_compact if compact else a.push)(x, starts, cnt, final=final)
        bq, slot, frames, start = b.live(rb)                      # (synchronises: a test)
        assert torch.equal(a.state, b.state), (tag, "state bytes")
        if not compact:                                           # the slot form on the compact object
            for k in ("frame_start", "n_frames", "dropped"):
                assert torch.equal(getattr(ra, k), getattr(rb, k)), (tag, k)
            la = a.live(ra)
            assert all(torch.equal(u, v) for u, v in zip(la, (bq, slot, frames, start))), tag
            return ra
        total = int(bq.numel())
        n0 = min(total, rows)
        assert ra.n_rows.tolist() == [n0, max(total - rows, 0)], (tag, ra.n_rows.tolist(), total)
        nf = rb.n_frames.to(torch.int64)
        assert torch.equal(ra.n_frames, rb.n_frames), (tag, "n_frames")
        assert torch.equal(ra.row0.to(torch.int64), torch.cumsum(nf, 0) - nf), (tag, "row0")
        assert torch.equal(ra.dropped, rb.dropped), (tag, "dropped")
        assert torch.equal(raw(ra.frames[:n0]), raw(frames[:n0])), (tag, "frames")
        assert torch.equal(ra.frame_start[:n0], start[:n0]), (tag, "frame_start")
        assert torch.equal(ra.frame_stream[:n0].to(torch.int64), bq[:n0]), (tag, "frame_stream")
        assert (ra.frame_start[n0:] == -1).all() and (ra.frame_stream[n0:] == -1).all(), (tag, "-1 beyond n_rows[0]")
        assert (raw(ra.frames[n0:]) == PATTERN).all(), (tag, "unused row written")
        self.n_rows.append([n0, total - n0])
        self.dropped += rb.dropped.cpu()
        for s, q in zip(bq.tolist(), start.tolist()):
            self.order.setdefault(s, []).append(q)
        return ra


def run_scenario(sc: cm.Scenario, chunks, x: np.ndarray, kind: str, rows=None, alternate=False):
    """One capture_model scenario through a Pair, every push also against the model.  rows: the capacity
    (default: room for everything).  alternate: every second push of the compact object is a slot-form push."""
    n_br = x.shape[1]
    rows = cm.B * sc.Q if rows is None else rows
    pr = Pair(cm.B, n_br, sc.F, sc.H, sc.Q, rows, kind, sc.offset)
    xd = torch.from_numpy(x).cuda()
    dl = cm.deliveries(sc, chunks)
    want = cm.run_model(sc, chunks, x)
    n = 0
    pushes = list(enumerate(chunks)) + ([(None, 0)] if sc.flush else [])
    for i, (p, c) in enumerate(pushes):
        compact = not (alternate and i % 2 == 1)
        tag = (sc.name, kind, n_br, i)
        if p is not None and p in sc.resets:
            mask = torch.zeros(cm.B, dtype=torch.bool)
            mask[sc.resets[p]] = True
            pr.reset(mask)
        if p is None:
            r = pr.push(xd, flush=True, tag=tag, compact=compact)
        else:
            K = max(1, max(len(v) for v in dl[p]))
            ev = np.full((cm.B, K, 4), -(1 << 40), dtype=np.int64)               # a padding value is always late
            cnt = np.zeros(cm.B, dtype=np.int32)
            for b, vals in enumerate(dl[p]):
                ev[b, :len(vals), 3] = vals
                cnt[b] = len(vals) + (sc.over_count if len(vals) == K else 0)
            fin = sc.final and p == len(chunks) - 1
            if any(dl[p]) or sc.over_count:
                r = pr.push(xd[:, :, n:n + c], torch.from_numpy(ev).cuda()[:, :, 3], torch.from_numpy(cnt).cuda(),
                            final=fin, tag=tag, compact=compact)
            else:
                r = pr.push(xd[:, :, n:n + c], final=fin, tag=tag, compact=compact)
            n += c
        if not compact:
            continue
        # the model's rows of this push, (stream, slot) order, cut to the capacity
        exp = [(b, s, fr) for b, (starts, frames, _) in enumerate(want[i]) for s, fr in zip(starts, frames)]
        assert r.n_frames.tolist() == [len(o[0]) for o in want[i]], tag
        assert r.dropped.tolist() == [o[2] for o in want[i]], tag
        assert r.n_rows.tolist() == [min(len(exp), rows), max(len(exp) - rows, 0)], tag
        exp = exp[:rows]
        assert r.frame_stream[:len(exp)].tolist() == [e[0] for e in exp], tag
        assert r.frame_start[:len(exp)].tolist() == [e[1] for e in exp], tag
        if exp:
            fr = torch.from_numpy(np.ascontiguousarray(np.stack([e[2] for e in exp])))
            assert torch.equal(raw(r.frames[:len(exp)]).cpu(), raw(fr)), tag
    return pr


def busy_scenario(F: int, Q: int, seed: int) -> cm.Scenario:
    """Many triggers per stream around each delivery point: some late, some ahead of the stream, several per
    push (queue full at small Q, several frames per call at large Q).  The model decides what comes out."""
    H = F + 11
    T = 6 * H + 3 * F + 40
    rng = np.random.default_rng(seed)
    tr = []
    for d in sorted(rng.integers(0, T, size=14).tolist()):
        for b in rng.choice(cm.B, size=3, replace=False).tolist():
            for _ in range(int(rng.integers(1, 5))):
                tr.append((b, int(d + rng.integers(-H - 2, 4)), d))
    return cm.Scenario(f"busy_F{F}_Q{Q}", F, H, Q, 0, T, tr)


@pytest.mark.parametrize("n_br", [1, 2])
@pytest.mark.parametrize("kind", list(KINDS))
def test_formats_frame_lengths_and_queue_depths(kind, n_br):
    emitted = late = full = 0
    for F in (1, 5, 37):
        for Q in (1, 3, 16):
            sc = busy_scenario(F, Q, seed=100 * F + Q)
            x = cm.make_stream(kind, n_br, sc.T, seed=F + Q)
            for name, chunks in cm.chunkings(sc.T, F, sc.H).items():
                if name == "one sample":
                    continue
                pr = run_scenario(sc, chunks, x, kind)
                emitted += sum(n for n, _ in pr.n_rows)
                late += int(pr.dropped[:, 0].sum())
                full += int(pr.dropped[:, 1].sum())
                assert all(lost == 0 for _, lost in pr.n_rows)
    assert emitted > 0 and late > 0 and full > 0                  # the cases the scenarios are for did occur


@pytest.mark.parametrize("kind", list(KINDS))
def test_clean_scenarios_over_every_chunking(kind):
    for F, H in (cm.SIZES[0], (7, 44), (64, 128)):
        sc = cm.clean_scenario(F, H)
        x = cm.make_stream(kind, 2, sc.T, seed=F + H)
        want = {b: [val + sc.offset for bb, val, _ in sc.triggers if bb == b] for b in range(cm.B)}
        for name, chunks in cm.chunkings(sc.T, F, H).items():
            pr = run_scenario(sc, chunks, x, kind)
            assert {b: pr.order.get(b, []) for b in range(cm.B)} == want, (F, H, name)
            assert pr.dropped.sum().item() == 0


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("sc", cm.edge_scenarios(), ids=lambda s: s.name)
def test_edges(sc, kind):
    """Late triggers, queue full, cut by the end (final and the Tc = 0 flush), several frames per stream in one
    call, reset in mid-frame."""
    for n_br in (1, 2):
        x = cm.make_stream(kind, n_br, sc.T, seed=7)
        pr = run_scenario(sc, sc.chunks, x, kind)
        assert sum(n for n, _ in pr.n_rows) > 0
        assert tuple(pr.dropped.sum(0).tolist()) == sc.expect_dropped


@pytest.mark.parametrize("sc", [s for s in cm.edge_scenarios() if s.name in
                                ("staggered_completions", "queue_stays_full", "flush_cuts", "reset_mid_frame")],
                         ids=lambda s: s.name)
def test_alternating_with_the_slot_form(sc):
    """push and push_compact in turn on one object: every push equals the form used alone (the yardstick
    object uses the slot form alone, the test above the compact form alone), the states stay equal bytes."""
    x = cm.make_stream("c64", 2, sc.T, seed=11)
    run_scenario(sc, sc.chunks, x, "c64", alternate=True)
    sc2 = busy_scenario(5, 3, seed=5)
    x = cm.make_stream("i16", 1, sc2.T, seed=12)
    run_scenario(sc2, cm.chunkings(sc2.T, 5, sc2.H)["primes"], x, "i16", alternate=True)


# ---------------------------------------------------------------------------------------------
# the count-and-scan: capacity, idle pushes, block edges (Tc = 64, F = 8)
# ---------------------------------------------------------------------------------------------
TC, F8 = 64, 8


def stream_batch(B, n_push, seed=0):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, 1, n_push * TC)) + 1j * rng.standard_normal((B, 1, n_push * TC))
    return torch.from_numpy(z.astype(np.complex64)).cuda()


def triggers(B, per_stream: dict, K):
    """starts [B, K] and counts [B] with stream b's list per_stream[b]."""
    st = np.zeros((B, K), dtype=np.int64)
    cnt = np.zeros(B, dtype=np.int32)
    for b, vals in per_stream.items():
        st[b, :len(vals)] = vals
        cnt[b] = len(vals)
    return torch.from_numpy(st).cuda(), torch.from_numpy(cnt).cuda()


@pytest.mark.parametrize("rows,want", [(10, ([10, 0], [5, 0])), (9, ([9, 1], [5, 0])), (1, ([1, 9], [1, 4]))])
def test_capacity(rows, want):
    """A push of 10 frames (two per stream) into 10, 9 and 1 rows, then a push of 5: a frame without a row is
    lost and counted, and the next push is unaffected."""
    B = cm.B
    x = stream_batch(B, 2)
    pr = Pair(B, 1, F8, F8, 2, rows)
    st, cnt = triggers(B, {b: [3 + b, 20 + b] for b in range(B)}, 2)
    r = pr.push(x[:, :, :TC], st, cnt, tag="first")
    assert r.n_rows.tolist() == want[0] and r.n_frames.tolist() == [2] * B
    st, cnt = triggers(B, {b: [TC + 9 + b] for b in range(B)}, 2)
    r = pr.push(x[:, :, TC:], st, cnt, tag="second")
    assert r.n_rows.tolist() == want[1] and r.n_frames.tolist() == [1] * B
    assert r.frame_start[:want[1][0]].tolist() == [TC + 9 + b for b in range(want[1][0])]
    assert pr.dropped.sum().item() == 0                           # lost for want of a row is not `dropped`


def test_pushes_in_which_no_stream_emits():
    B = 7
    x = stream_batch(B, 3)
    pr = Pair(B, 1, F8, 2 * TC, 2, 5)
    r = pr.push(x[:, :, :TC], tag="no triggers")
    assert r.n_rows.tolist() == [0, 0] and (r.frame_start == -1).all() and (r.frame_stream == -1).all()
    assert r.row0.tolist() == [0] * B and r.n_frames.tolist() == [0] * B
    st, cnt = triggers(B, {2: [2 * TC - 3], 5: [2 * TC + 1]}, 1)   # complete only in the third push
    r = pr.push(x[:, :, TC:2 * TC], st, cnt, tag="pending only")
    assert r.n_rows.tolist() == [0, 0] and (r.frame_start == -1).all() and (r.frame_stream == -1).all()
    r = pr.push(x[:, :, 2 * TC:], tag="they complete")
    assert r.n_rows.tolist() == [2, 0] and r.frame_stream.tolist() == [2, 5, -1, -1, -1]
    assert r.row0.tolist() == [0, 0, 0, 1, 1, 1, 2]


def _scan_case(B, emitters: dict, rows):
    x = stream_batch(B, 1, seed=B)
    pr = Pair(B, 1, F8, F8, 4, rows)
    st, cnt = triggers(B, emitters, 4)
    r = pr.push(x, st, cnt, tag=("scan", B))
    total = sum(len(v) for v in emitters.values())
    assert r.n_rows.tolist() == [total, 0]
    return r


def test_scan_block_edges():
    """B = 1, the scan's block size - 1, the block size, + 1: frames in the first stream, around the block
    boundary and in the last stream, in unequal numbers (a prefix that is wrong across the boundary shows)."""
    from ofdm_sync_amd.capture import SCAN_BLOCK as S
    r = _scan_case(1, {0: [5, 9, 30]}, 4)
    assert r.frame_start.tolist() == [5, 9, 30, -1] and r.frame_stream.tolist() == [0, 0, 0, -1]
    for B in (S - 1, S, S + 1):
        # (streams 3 | 4 and 255 | 256: neighbours in two threads and in two waves of the scan)
        em = {0: [1, 2], 3: [9], 4: [5, 6], 255: [7], 256: [3, 4, 5], B - 2: [11], B - 1: [8, 40]}
        if B > S:
            em[S - 1] = [6, 7, 8, 9]
        r = _scan_case(B, em, 20)
        assert r.row0[B - 1].item() == sum(len(v) for b, v in em.items() if b < B - 1)


def test_scan_over_three_blocks_first_and_last_stream_only():
    from ofdm_sync_amd.capture import SCAN_BLOCK as S
    B = 2 * S + 5
    r = _scan_case(B, {0: [3, 17], B - 1: [21]}, 8)
    assert r.frame_stream[:3].tolist() == [0, 0, B - 1] and r.frame_start[:3].tolist() == [3, 17, 21]
    assert r.row0[1].item() == 2 and r.row0[S].item() == 2 and r.row0[2 * S].item() == 2 and r.row0[B - 1].item() == 2


def test_scan_with_frames_in_every_stream():
    from ofdm_sync_amd.capture import SCAN_BLOCK as S
    B = 2 * S + 5
    em = {b: [1 + (b % 50) + 3 * j for j in range(1 + b % 3)] for b in range(B)}
    total = sum(len(v) for v in em.values())
    r = _scan_case(B, em, total + 3)
    assert r.n_frames.tolist() == [1 + b % 3 for b in range(B)]
    # ... and into fewer rows than frames: the cut falls inside a stream of the second block
    x = stream_batch(B, 1, seed=B)
    rows = sum(len(em[b]) for b in range(S + 10)) + 1
    pr = Pair(B, 1, F8, F8, 4, rows)
    st, cnt = triggers(B, em, 4)
    r = pr.push(x, st, cnt, tag="cut")
    assert r.n_rows.tolist() == [rows, total - rows]


def test_python_refusals():
    from ofdm_sync_amd.capture import FrameCapture, StreamReceiver
    x = torch.zeros((2, 1, 4), dtype=torch.complex64, device="cuda")
    cap = FrameCapture(2, 1, frame_len=8)
    with pytest.raises(ValueError):
        cap.push_compact(x)                                       # made without compact_rows
    with pytest.raises(ValueError):
        StreamReceiver(cap, 0, 4, np.ones(2), np.ones(2), n_fft=4, cp_len=0, fs_hz=1.0, bins=[-1, 1])
    for rows in (0, -1, 1 << 31):
        with pytest.raises(ValueError):
            FrameCapture(2, 1, frame_len=8, compact_rows=rows)
    cap = FrameCapture(2, 1, frame_len=8, compact_rows=3)
    with pytest.raises(ValueError):
        cap.push_compact(x[:, :, :0])                             # empty chunk without final
    r = cap.push_compact(x[:, :, :0], final=True)                 # the flush
    assert r.n_rows.tolist() == [0, 0] and tuple(r.frames.shape) == (3, 1, 8)
