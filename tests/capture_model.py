"""Plain-Python model of ofs_frame_capture_chunk (include/ofdmsync.h) and the trigger scenarios that
tests/test_capture_model_host.py (CPU) and tests/test_gpu_frame_capture.py (GPU) share.

The model follows the header's rules literally: per stream a count of samples, the last ``history``
samples (exactly H, no rounding), a queue of pending starts; triggers first, then the queue, then
``final``, then the history.  A frame is read from [history | chunk] and the model fails loudly if a
sample it needs is in neither: that is the retrievability argument (H >= F), checked and not assumed.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


class CaptureModel:
    def __init__(self, B: int, n_br: int, F: int, H: int, Q: int, offset: int = 0):
        assert F >= 1 and H >= F and 1 <= Q <= 16
        self.B, self.n_br, self.F, self.H, self.Q, self.offset = B, n_br, F, H, Q, offset
        self.n = [0] * B
        self.pend = [[] for _ in range(B)]
        self.hist = [None] * B                       # [n_br, <= H] samples before n

    def reset(self, streams):
        for b in streams:
            self.n[b], self.pend[b], self.hist[b] = 0, [], None

    def push(self, x, trig=None, final=False):
        """x: [B, n_br, Tc(, 2)] numpy (Tc may be 0 with final); trig: per stream a list of trigger values
        (None: no triggers).  Returns per stream (starts [<= Q], frames [len(starts), n_br, F(, 2)],
        dropped [late, full, cut])."""
        Tc = x.shape[2]
        assert Tc > 0 or final
        out = []
        for b in range(self.B):
            n0, n1 = self.n[b], self.n[b] + Tc
            hist = self.hist[b] if self.hist[b] is not None else x[b][:, :0]
            late = full = cut = 0
            for t in (trig[b] if trig is not None else ()):
                s = int(t) + self.offset
                if s < max(0, n0 - self.H):
                    late += 1
                elif len(self.pend[b]) >= self.Q:
                    full += 1
                else:
                    self.pend[b].append(s)
            both = np.concatenate([hist, x[b]], axis=1)         # samples [n0 - hist_len, n1)
            base = n0 - hist.shape[1]
            starts, frames, keep = [], [], []
            for s in self.pend[b]:
                if s + self.F <= n1:
                    assert s >= base, f"stream {b}: start {s} left the history (oldest {base})"
                    starts.append(s)
                    frames.append(both[:, s - base:s - base + self.F])
                else:
                    keep.append(s)
            assert len(starts) <= self.Q
            self.pend[b] = keep
            if final:
                cut = len(keep)
                self.n[b], self.pend[b], self.hist[b] = 0, [], None
            else:
                self.n[b], self.hist[b] = n1, both[:, max(0, both.shape[1] - self.H):]
            fr = np.stack(frames) if frames else x[b][None, :, :0][:0]
            out.append((starts, fr, [late, full, cut]))
        return out


# ---------------------------------------------------------------------------------------------
# scenarios: a trigger is (stream, value, d) - the value reaches the capture in the push that holds
# sample d of the stream (n0 <= d < n1), as a detector's event would
# ---------------------------------------------------------------------------------------------
@dataclass
class Scenario:
    name: str
    F: int
    H: int
    Q: int
    offset: int
    T: int
    triggers: list                                   # (stream, value, d), in delivery order within a push
    chunks: list | None = None                       # fixed chunking (edge scenarios); None: any
    final: bool = False                              # the last push is final
    flush: bool = False                              # a flush() after the last push
    resets: dict = field(default_factory=dict)       # push index -> streams reset BEFORE that push
    over_count: int = 0                              # n_starts handed in = count + over_count (above trig_max)
    expect_dropped: tuple | None = None              # total (late, full, cut) over all streams and pushes


B = 5
SIZES = [(F, H) for F in (1, 7, 64, 300) for H in (F, F + 37, 2 * F)]


def clean_scenario(F: int, H: int) -> Scenario:
    """Triggers that are never late, never find the queue full and complete before the end, for ANY
    chunking, and whose frames leave each stream in one order for any chunking (each stream's triggers
    complete in the order they are queued).  Q = 4, offset = -3."""
    Q, off = 4, -3
    T = 5 * H + 2 * F + 11
    tr = []
    v = lambda s: s - off                            # noqa: E731  the trigger value of start s
    # stream 0: delivered in the push that holds the frame's first sample; a second, overlapping frame
    s0 = 2 * H + H // 3 + 1
    tr += [(0, v(s0), s0), (0, v(s0 + F // 2), s0 + F // 2)]
    # stream 1: delivered as late as retention allows (one-sample pushes: s == n0 - H exactly)
    s1 = 3 * H + 2
    tr += [(1, v(s1), s1 + H)]
    # stream 2: every residue of s mod 4, each delivered when its frame is complete
    s2 = 4 * H + 1
    tr += [(2, v(s2 + r), s2 + r + F) for r in range(4)]
    # stream 3: idle
    # stream 4: three triggers in one delivery, unsorted, all complete (s <= d - F) and retained (s >= d - H)
    d4 = H + F + 5
    tr += [(4, v(d4 - F), d4), (4, v(d4 - H), d4), (4, v(d4 - F), d4)]
    assert all(0 <= d < T and val + off + F <= T and val + off >= 0 for _, val, d in tr)
    return Scenario(f"clean_F{F}_H{H}", F, H, Q, off, T, tr, expect_dropped=(0, 0, 0))


def chunkings(T: int, F: int, H: int) -> dict:
    """name -> list of chunk lengths summing to T."""
    def fill(lengths):
        out, n, i = [], 0, 0
        while n < T:
            c = min(lengths[i % len(lengths)], T - n)
            out.append(c)
            n += c
            i += 1
        return out
    ch = {"primes": fill([7, 13, 31, 101, 3, 2, 61]), "Tc=H": fill([H]), "Tc>H": fill([H + 19, 2 * H + 1]),
          "one push": [T]}
    if (F, H) == SIZES[0]:
        ch["one sample"] = [1] * T
    return ch


def edge_scenarios() -> list:
    """Fixed chunkings that hit each rule's edge on purpose (F = 7, H = 12 unless said).  The totals in
    ``expect_dropped`` are worked out by hand from the rules, not from the model."""
    F, H = 7, 12
    sc = []
    # frame ending exactly at the chunk's end (stream 0) and one sample later (stream 1): pushes end at 20, 21
    sc.append(Scenario("ends_at_chunk_end", F, H, 2, 0, 40, [(0, 13, 14), (1, 14, 14)], chunks=[14, 6, 1, 19],
                       expect_dropped=(0, 0, 0)))
    # retention edge in the push with n0 = 30: s = 18 = n0 - H is kept, s = 17 is late; s = -1 in the first
    # push and s = -2 later are late (negative); stream 3: offset makes a valid value negative
    sc.append(Scenario("retention_edge", F, H, 2, 0, 50, [(0, 18, 30), (1, 17, 30), (2, -1, 0), (2, -2, 30)],
                       chunks=[30, 20], expect_dropped=(3, 0, 0)))
    sc.append(Scenario("offset_below_zero", F, H, 2, -5, 50, [(3, 4, 0), (3, 5, 0)], chunks=[30, 20],
                       expect_dropped=(1, 0, 0)))
    # Q + 1 = 3 triggers in one call: the third finds the queue full; the two frames complete in that call
    sc.append(Scenario("queue_full", F, H, 2, 0, 40, [(0, 20, 25), (0, 22, 25), (0, 24, 25)], chunks=[10, 30],
                       expect_dropped=(0, 1, 0)))
    # ... and with the queue still full in the next call: two pending (incomplete), one more trigger is dropped
    sc.append(Scenario("queue_stays_full", F, H, 2, 0, 60, [(1, 28, 25), (1, 29, 25), (1, 30, 31)],
                       chunks=[20, 10, 3, 27], expect_dropped=(0, 1, 0)))
    # several frames completing in one call, Q = 16, overlapping, every residue mod 4 and mod 2
    sc.append(Scenario("staggered_completions", F, 40, 16, 0, 120, [(2, 50 + r, 50 + r) for r in range(16)],
                       chunks=[50, 5, 5, 6, 54], expect_dropped=(0, 0, 0)))
    sc.append(Scenario("sixteen_in_one_call", F, 40, 16, 0, 120, [(2, 50 + r, 70) for r in range(16)],
                       chunks=[50, 5, 5, 6, 54], expect_dropped=(0, 0, 0)))
    # n_trig above trig_max: the surplus is ignored, not read
    sc.append(Scenario("count_above_max", F, H, 4, 0, 40, [(0, 5, 12), (4, 6, 12), (4, 8, 12)], chunks=[10, 30],
                       over_count=7, expect_dropped=(0, 0, 0)))
    # final with a start pending (stream 0: needs sample 45) while stream 1's frame ends exactly at the end
    sc.append(Scenario("final_cuts", F, H, 2, 0, 40, [(0, 39, 30), (1, 33, 30)], chunks=[25, 15], final=True,
                       expect_dropped=(0, 0, 1)))
    # flush() with Tc = 0: two starts pending in stream 2, one in stream 3 (stream 0's frame is complete before)
    sc.append(Scenario("flush_cuts", F, H, 2, 0, 40, [(0, 20, 30), (2, 36, 30), (2, 38, 30), (3, 34, 30)],
                       chunks=[25, 15],
                       flush=True, expect_dropped=(0, 0, 3)))
    # reset(mask) of streams 1 and 3 in mid-frame (before push 2): their starts are forgotten without a
    # count and they restart at sample 0 (stream 3 then gets a frame at its new index 2); 0, 2, 4 go on
    sc.append(Scenario("reset_mid_frame", F, H, 2, 0, 60,
                       [(0, 18, 18), (1, 18, 18), (2, 17, 18), (3, 19, 18), (3, 2, 30)],
                       chunks=[20, 3, 10, 27], resets={2: [1, 3]}, expect_dropped=(0, 0, 0)))
    return sc


def deliveries(sc: Scenario, chunks: list) -> list:
    """Per push, per stream: the list of trigger values delivered.  After a reset a stream counts its
    samples from 0 again, but d stays the stream's index in the test's whole array."""
    bounds = np.concatenate([[0], np.cumsum(chunks)])
    out = [[[] for _ in range(B)] for _ in chunks]
    for b, val, d in sc.triggers:
        p = int(np.searchsorted(bounds, d, side="right")) - 1
        assert 0 <= p < len(chunks), (sc.name, b, val, d)
        out[p][b].append(val)
    return out


def run_model(sc: Scenario, chunks: list, x: np.ndarray):
    """The model over one chunking of x [B, n_br, T(, 2)].  Returns per push the model's output (the
    flush, if any, as one more push), and per stream the base index of its current numbering at each push."""
    m = CaptureModel(B, x.shape[1], sc.F, sc.H, sc.Q, sc.offset)
    dl = deliveries(sc, chunks)
    outs, n = [], 0
    for p, c in enumerate(chunks):
        if p in sc.resets:
            m.reset(sc.resets[p])
        outs.append(m.push(x[:, :, n:n + c], dl[p], final=sc.final and p == len(chunks) - 1))
        n += c
    if sc.flush:
        outs.append(m.push(x[:, :, :0], None, final=True))
    return outs


def make_stream(kind: str, n_br: int, T: int, seed: int = 0) -> np.ndarray:
    """Random samples [B, n_br, T(, 2)]: 'c64' | 'c128' complex, 'i16' int16 I/Q pairs."""
    rng = np.random.default_rng(seed)
    if kind == "i16":
        return rng.integers(-32768, 32768, size=(B, n_br, T, 2), dtype=np.int16)
    z = rng.standard_normal((B, n_br, T)) + 1j * rng.standard_normal((B, n_br, T))
    return z.astype(np.complex64 if kind == "c64" else np.complex128)
