"""Exact |corr| streams for the zc_v2 CFAR + gate (csrc/zc_cfar.hip, zc_detect_kernel of csrc/corr.hip).

NumPy and the CPU oracle only.  Every sample is a multiple of 2^-4 in [0, 4] and n <= 2304, so every
running sum is below 2^14 with 4 fractional bits: the reference's float64 recursion (acc + c[i]) - c[i-W]
is exact in any order, c * 2^f and local_sum * tv are exact integers, and equality in the CFAR
comparison is real.  Expected results always come from ofdm_oracle.zc_streaming_detection and
ofdm_oracle.detect_zc_peaks (expected()), never from the pattern a stream was built from.

Two families, one batch each (a launch takes one parameter set):
  M  min_corr_mag decides: thresh_value 1, thresh_frac_bits 15, min_corr_mag 0.5, baseline 0.125,
     above samples 0.5, 1.0 or 2.0.  c >= 0.5 gives c * 2^15 >= 2^14 > local_sum, so
     above == valid & (c >= 0.5) and the above pattern is placed sample by sample.
  C  the CFAR comparison decides: min_corr_mag 0, thresh_value 2^(15 - m) with 2^m the largest power of
     two below W, values in {1 .. 16} / 16.  With s the sum of the W - 1 samples before sample i and
     D = 2^m - 1, sample i is above iff c16 * D >= s (c16 = 16 c): the streams hold samples on the tie
     c16 * D == s (above), one step under it (not above), and large non-above samples inside an open
     gate, including the largest value of a gate on a non-above sample and on the closing sample.

streams(n, W, hyst) -> {"M": Batch, "C": Batch}; check(n, W, hyst) asserts exactness and the coverage
of the gate machine's edges; MUTANTS are small wrong variants of the two oracle functions, each of which
must change flags, mask or events on a stream (mutants_caught).
"""
import functools
from collections import namedtuple

import numpy as np

import ofdm_oracle as O

FRAC_BITS = 15
REFLEN = 100                       # reference_length of every call: detected_start clips at 0 for early peaks
N_MAX = 2304
MIN_STREAMS = 33

# (n, W) of tests/test_gpu_zc_exact_events.py and the hysteresis lists of the two kernels
SHAPES = ((1024, 128), (1152, 256), (2304, 1024), (1000, 128), (1024, 100), (130, 128), (128, 128), (64, 32))
DMA_SHAPES = ((1024, 128), (1152, 256), (2304, 1024), (128, 128))
HYSTS_SEQ = (0, 1, 2, 63)


def hysts_fused(n):
    return (64, 65, 127, 128, 129, 256, 1000, n + 7)


def all_cases():
    return [(n, W, h) for n, W in SHAPES for h in hysts_fused(n) + HYSTS_SEQ]


# params: window_size, thresh_value, thresh_frac_bits, min_corr_mag (the oracle's argument order)
Batch = namedtuple("Batch", "names c params")


def c_shift(W):
    """m of family C: 2^m is the largest power of two below W (D = 2^m - 1 <= W - 2)."""
    return max(1, int(np.ceil(np.log2(W))) - 1)


# ------------------------------------------------------------------------------------------
# family M
# ------------------------------------------------------------------------------------------
def _m(n, pairs):
    c = np.full(n, 0.125)
    for i, v in pairs:
        if 0 <= i < n:
            c[i] = v
    return c


def _first(lo, r, mod):
    """Smallest p >= lo with p % mod == r % mod."""
    return lo + (r - lo) % mod


def _chain(n, start, gaps):
    out, p, k = [], start, 0
    while p < n:
        out.append((p, 1.0))
        p += gaps[k % len(gaps)]
        k += 1
    return out


def family_m(n, W, hyst):
    Hp = max(hyst, 1)
    names, rows = [], []

    def add(name, pairs):
        names.append(name)
        rows.append(_m(n, pairs))

    add("silent", [])
    add("all_above", [(i, 1.0) for i in range(n)])
    # samples >= 0.5 before i = W (larger than anything later) are ignored; first above exactly at W
    add("pre_valid", [(i, 2.0) for i in range(W)] + [(W, 1.0)])
    # single above samples at gaps Hp - 1, Hp, Hp + 1, started at offsets that move the edges through a row
    gaps = [g for g in (Hp - 1, Hp, Hp + 1) if g >= 1]
    for d in (0, 1, 63, 64, 65, 127):
        add(f"chain+{d}", _chain(n, W + d, gaps))
    # lone pulses: gate_end = p + Hp and gate_start = p on the first / last lane of a row and of a chunk
    for r in (0, 63, 64, 127):
        add(f"end%128={r}", [(_first(W + 1, r - Hp, 128), 1.0)])
    for r in (0, 63, 64, 127):
        add(f"start%128={r}", [(_first(W + 1, r, 128), 1.0)])
    # close at p + Hp, reopen on the next sample: inside a row, across rows, across chunks
    for r in (0, 10, 63, 127):
        p = _first(W + 1, r - Hp, 128)
        add(f"reopen%128={r}", [(p, 1.0), (p + Hp + 1, 1.0)])
    # the minimal chain: every gate is one above sample and closes Hp later (Hp = 64: two closes per chunk)
    add("min_chain", _chain(n, W, [Hp + 1]))
    # tails: last_above + Hp = n - 1 (close on the last sample), n, n + 1 (left open), above at n - 1
    for k, t in (("n-1", n - 1 - Hp), ("n", n - Hp), ("n+1", n + 1 - Hp)):
        add(f"tail_close_at_{k}", [(t, 1.0)] if t >= W else [])
    add("tail_above_last", [(n - 1, 1.0)] if n - 1 >= W else [])
    # peak ties inside one long gate (a block of above samples): equal maxima in different rows, in
    # different chunks, and the opening sample tied with a later one
    p = W + 3
    blk = [(i, 1.0) for i in range(p, min(n, p + 200))]
    add("tie_rows", blk + [(p + 5, 2.0), (p + 5 + 64, 2.0)])
    add("tie_chunks", blk + [(p + 5, 2.0), (p + 5 + 128, 2.0)])
    add("tie_open", blk + [(p, 2.0), (p + 130, 2.0)])
    # exact equality with min_corr_mag
    add("min_tie", [(W + 7, 0.5), (W + 7 + Hp + 1, 0.5)])
    return Batch(names, np.array(rows).reshape(len(names), n), (W, 1, FRAC_BITS, 0.5))


# ------------------------------------------------------------------------------------------
# family C
# ------------------------------------------------------------------------------------------
class _CB:
    """Greedy builder in units of 2^-4: s() is the sum of the W - 1 samples before the next one, and the
    next sample is above iff c16 * D >= s()."""

    def __init__(self, n, W):
        self.n, self.W, self.D = n, W, (1 << c_shift(W)) - 1
        self.v = []

    @property
    def i(self):
        return len(self.v)

    def s(self):
        return sum(self.v[max(0, self.i - self.W + 1):])

    def put(self, c16):
        assert 1 <= c16 <= 16
        if self.i < self.n:
            self.v.append(int(c16))

    def low(self):
        self.put(1)

    def big_max(self):
        """Largest non-above value of the next sample (0: none)."""
        return min(16, (self.s() - 1) // self.D)

    def above_min(self):
        return -(-self.s() // self.D)

    def done(self):
        while self.i < self.n:
            self.low()
        return np.array(self.v[:self.n], np.float64) / 16.0


def _prefix_sum_to(W, total):
    """W samples in 1..16 whose last W - 1 sum to `total` (the window of sample W)."""
    v = [1] * W
    extra = total - (W - 1)
    assert 0 <= extra <= 15 * (W - 1)
    for k in range(1, W):
        a = min(15, extra)
        v[k] += a
        extra -= a
    return v


def _c_gate_peak(n, W, Hp, close):
    """A gate opened at i = W whose largest value lies on a non-above sample: in the gate's interior
    (close False) or on its closing sample W + Hp (close True).  The window of sample W holds K - 1 ones
    (they leave first) and W - K samples of level h, chosen so that the opener is an exact tie; non-above
    samples as large as allowed (capped at the opener's value: ties with it) then raise the sum until a
    larger value is still not above.  None when no (h, K) gives one inside [W, n)."""
    if W + (Hp if close else 2) > n - 1:
        return None
    for h in range(15, 1, -1):
        for K in range(2, W):
            b = _CB(n, W)
            s0 = K - 1 + (W - K) * h
            if s0 % b.D or not 2 <= s0 // b.D <= 14:
                continue
            a = s0 // b.D
            b.v = [1] * K + [h] * (W - K)
            b.put(a)                                           # the opener at i = W: tie, above
            ok = False
            while b.i < min(n, W + Hp + 1):
                last = b.i == W + Hp                           # the closing sample (no above since W)
                m = b.big_max()
                if m < 1:
                    break
                if (last or not close) and m > a:
                    b.put(m)
                    ok = last == close
                    break
                if last:
                    break
                b.put(min(m, a))
            if ok:
                return b.done()
    return None


def family_c(n, W, hyst):
    Hp = max(hyst, 1)
    D = (1 << c_shift(W)) - 1
    names, rows = [], []

    def add(name, c):
        names.append(name)
        rows.append(c)

    add("c_silent", _CB(n, W).done())
    # the first valid sample on the tie (above: a gate from W), and one step under it (not above)
    for name, dv in (("c_tie_at_W", 0), ("c_under_at_W", -1)):
        b = _CB(n, W)
        b.v = _prefix_sum_to(W, 3 * D)[:n]
        if n > W:
            assert b.s() == 3 * D
            b.put(3 + dv)
        add(name, b.done())
    # a tie and a sample under the tie reached from a quiet window (W a power of two: a sample of 2 / 16 is
    # still not above a window of ones, so 2s walk the sum up to 3 D)
    b = _CB(n, W)
    if W == 2 * (D + 1) and 2 * W + 2 * D + 8 <= n:
        b.v = [1] * (2 * W)                                    # the sum is W - 1 = 2 D + 1; each 2 adds one
        while b.s() < 3 * D:
            b.put(2)
        b.put(2)                                               # one step under the tie at 3
        while b.s() < 4 * D:
            b.put(2)
        assert b.s() == 4 * D and b.i < n
        b.put(4)                                               # the tie
    add("c_quiet_tie", b.done())
    for name, close in (("c_peak_non_above", False), ("c_peak_on_close", True)):
        c = _c_gate_peak(n, W, Hp, close)
        add(name, c if c is not None else _CB(n, W).done())
    return Batch(names, np.array(rows).reshape(len(names), n), (W, 1 << (FRAC_BITS - c_shift(W)), FRAC_BITS, 0.0))


@functools.lru_cache(maxsize=None)
def streams(n, W, hyst):
    """The two batches of (n, W, hyst); arrays are read-only (shared by every test)."""
    assert n <= N_MAX
    out = {"M": family_m(n, W, hyst), "C": family_c(n, W, hyst)}
    for bt in out.values():
        bt.c.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------
# expected results: the oracle, and its mutants
# ------------------------------------------------------------------------------------------
def run_oracle(c, params, hyst, reflen=REFLEN):
    W, tv, f, mn = params
    st = O.zc_streaming_detection(c, W, tv, f, mn)
    ev, val, mask = O.detect_zc_peaks(c, st["above_threshold"], st["metric_valid"], reflen, hyst)
    return dict(st, events=ev, peak_values=val, gate_mask=mask)


@functools.lru_cache(maxsize=None)
def expected(n, W, hyst):
    """{"M": [per-stream oracle dict], "C": [...]} for streams(n, W, hyst)."""
    return {k: [run_oracle(bt.c[b], bt.params, hyst) for b in range(len(bt.names))]
            for k, bt in streams(n, W, hyst).items()}


def run_mutant(c, params, hyst, mut):
    """The two oracle functions restated with one deliberate error `mut` (None: no error; the result then
    equals run_oracle, which check() asserts).  Rows are 64 samples and chunks 128, as in zc_cfar.hip."""
    W, tv, f, mn = params
    W = max(1, int(W))
    c = np.asarray(c, np.float64)
    n = c.size
    local = np.zeros(n)
    acc = 0.0
    for i in range(n):
        acc = acc + c[i] - c[i - W] if i >= W else acc + c[i]
        local[i] = acc
    v0 = {"valid_from_W-1": W - 1, "valid_from_W+1": W + 1}.get(mut, W)
    valid = np.arange(n) >= v0
    cs, ts = c * float(1 << f), local * float(tv)
    above = valid & ((cs > ts) if mut == "cfar_gt" else (cs >= ts)) & ((c > mn) if mut == "min_gt" else (c >= mn))
    mask = np.zeros(n, bool)
    evs, vals = [], []
    is_open = False
    gs = pk = low = 0
    pv = 0.0
    lim = max(0, hyst - 1) + {"close_early": -1, "close_late": 1}.get(mut, 0)
    carried = False                    # a gate was open at the start of this 64-row
    closes = 0                         # closes in this 128-chunk
    for i in range(n):
        if i % 64 == 0:
            carried = is_open
        if i % 128 == 0:
            closes = 0
            quiet = mut == "quiet_ignores_open_gate" and not above[i:i + 128].any()
        if not valid[i] or quiet:
            continue
        v = c[i]
        if not is_open:
            if above[i] and not (mut == "no_reopen_in_close_row" and carried):
                is_open, gs, pk, low = True, i, i, 0
                pv = -np.inf if mut == "open_not_in_peak" else v
                if mut == "open_in_mask":
                    mask[i] = True
        else:
            mask[i] = True
            closing = (not above[i]) and (hyst == 0 or low >= lim) and not (mut == "one_close_per_chunk" and closes)
            if (v >= pv if mut == "peak_ge" else v > pv) and not (mut == "close_not_in_peak" and closing):
                pv, pk = v, i
            if above[i]:
                low = 0
            elif closing:
                evs.append((pk, gs, i, max(0, pk - REFLEN + 1)))
                vals.append(pv)
                is_open, pv, low = False, 0.0, 0
                closes += 1
            else:
                low += 1
    if is_open:
        evs.append((pk, gs, n - 1 if mut == "open_end_n-1" else n, max(0, pk - REFLEN + 1)))
        vals.append(pv)
        mask[gs:n] = True
    return dict(corr_mag=c, local_sum=local, corr_scaled=cs, thresh_scaled=ts, above_threshold=above,
                metric_valid=valid, events=np.array(evs, np.int64).reshape(-1, 4),
                peak_values=np.array(vals, np.float64), gate_mask=mask)


# name -> arithmetic predicate on Hp under which the mutant can differ from the oracle at all.  Two closes
# lie at least Hp + 1 samples apart (a gate needs an above sample, then Hp samples to close), so a
# 128-sample chunk holds two of them only when Hp + 1 <= 127: "one_close_per_chunk" IS the oracle for
# Hp >= 127, on every stream.  Every other mutant must be caught at every Hp.
MUTANTS = {
    "close_early": lambda Hp: True,
    "close_late": lambda Hp: True,
    "no_reopen_in_close_row": lambda Hp: True,
    "one_close_per_chunk": lambda Hp: Hp + 1 <= 127,
    "quiet_ignores_open_gate": lambda Hp: True,
    "peak_ge": lambda Hp: True,
    "close_not_in_peak": lambda Hp: True,
    "open_not_in_peak": lambda Hp: True,
    "valid_from_W-1": lambda Hp: True,
    "valid_from_W+1": lambda Hp: True,
    "cfar_gt": lambda Hp: True,
    "min_gt": lambda Hp: True,
    "open_in_mask": lambda Hp: True,
    "open_end_n-1": lambda Hp: True,
}
DECISIONS = ("above_threshold", "metric_valid", "gate_mask", "events", "peak_values")


def same_decisions(a, b):
    return all(np.array_equal(a[k], b[k]) for k in DECISIONS)


def mutants_caught(n, W, hyst):
    """{mutant: [names of the streams on which it changes flags, mask or events]}."""
    st, exp = streams(n, W, hyst), expected(n, W, hyst)
    out = {}
    for mut in MUTANTS:
        out[mut] = [bt.names[b] for k, bt in st.items() for b in range(len(bt.names))
                    if not same_decisions(run_mutant(bt.c[b], bt.params, hyst, mut), exp[k][b])]
    return out


# ------------------------------------------------------------------------------------------
# check(): preconditions and coverage
# ------------------------------------------------------------------------------------------
def _exact(bt, exp, hyst):
    """The oracle's state equals int64 arithmetic on c * 16 (and run_mutant without a mutation)."""
    W, tv, f, mn = bt.params
    c16f = bt.c * 16.0
    assert np.all(c16f == np.round(c16f)) and c16f.min() >= 0 and c16f.max() <= 64
    c16 = c16f.astype(np.int64)
    n = c16.shape[1]
    for b, name in enumerate(bt.names):
        cum = np.concatenate(([0], np.cumsum(c16[b])))
        i = np.arange(n)
        ls16 = cum[i + 1] - cum[np.maximum(i + 1 - W, 0)]
        e = exp[b]
        assert np.array_equal(e["local_sum"] * 16.0, ls16.astype(np.float64)), name
        valid = i >= W
        above = valid & ((c16[b] << f) >= ls16 * tv) & (c16[b] >= int(mn * 16))
        assert np.array_equal(e["metric_valid"], valid) and np.array_equal(e["above_threshold"], above), name
        assert np.array_equal(e["corr_scaled"], (c16[b] << f) / 16.0), name
        assert np.array_equal(e["thresh_scaled"], (ls16 * tv) / 16.0), name
        if mn > 0:
            assert np.array_equal(above, valid & (bt.c[b] >= 0.5)), name
        assert same_decisions(run_mutant(bt.c[b], bt.params, hyst, None), e), name


def facts(n, W, hyst):
    """Coverage facts present in the oracle's output for streams(n, W, hyst), as a set of names."""
    Hp = max(hyst, 1)
    st, exp = streams(n, W, hyst), expected(n, W, hyst)
    got = set()
    for k, bt in st.items():
        _, tv, f, _ = bt.params
        for b, name in enumerate(bt.names):
            e = exp[k][b]
            ev, ab, c = e["events"], e["above_threshold"], bt.c[b]
            ai = np.flatnonzero(ab)
            if len(ev) == 0:
                got.add("silent")
            if len(ev) == 1 and ev[0].tolist()[:3] == [W, W, n] and ab[W:].all():
                got.add("all_above")
            if len(ev) and ev[0, 1] == W and (c[:W] >= 0.5).any() and k == "M":
                got.add("pre_valid_ignored")
            if len(ev) and ev[0, 1] == W:
                got.add("first_valid_above")
            for g in np.diff(ai):
                for d in (-1, 0, 1):
                    if g == Hp + d:
                        got.add(f"gap_Hp{d:+d}")
            closed = ev[ev[:, 2] < n]
            for e_ in closed[:, 2]:
                got.update({f"end%64={e_ % 64}"} & {"end%64=0", "end%64=63"})
                got.update({f"end%128={e_ % 128}"} & {"end%128=0", "end%128=127"})
            for s_ in ev[:, 1]:
                got.update({f"start%64={s_ % 64}"} & {"start%64=0", "start%64=63"})
                got.update({f"start%128={s_ % 128}"} & {"start%128=0", "start%128=127"})
            for j in range(len(ev) - 1):
                if ev[j + 1, 1] == ev[j, 2] + 1:
                    got.add("reopen_next_chunk" if ev[j, 2] % 128 == 127 else
                            "reopen_next_row" if ev[j, 2] % 64 == 63 else "reopen_same_row")
            ch = closed[:, 2] // 128
            if len(ch) != len(set(ch.tolist())):
                got.add("two_closes_in_chunk")
            if len(ev) > 8:
                got.add("more_than_8_events")
            if len(ai):
                la = int(ai[-1])
                if la + Hp == n - 1 and len(ev) and ev[-1, 2] == n - 1:
                    got.add("close_on_last_sample")
                if la + Hp == n and ev[-1, 2] == n:
                    got.add("open_end_close_at_n")
                if la + Hp == n + 1 and ev[-1, 2] == n:
                    got.add("open_end_close_at_n+1")
                if la == n - 1:
                    got.add("above_at_n-1")
            for pk, gs, ge, _ in ev.tolist():
                seg = c[gs:min(ge, n - 1) + 1]
                at = gs + np.flatnonzero(seg == seg.max())
                assert pk == at[0]                              # the oracle: the first maximum
                if len(set((at // 64).tolist())) > 1:
                    got.add("tie_other_row")
                if len(set((at // 128).tolist())) > 1:
                    got.add("tie_other_chunk")
                if len(at) > 1 and pk == gs:
                    got.add("tie_with_opener")
                if not ab[pk] and pk != ge:
                    got.add("peak_non_above")
                if pk == ge and ge < n:
                    got.add("peak_on_close")
            if k == "C":
                # in integers: sample c16 against the sum s16 of the W - 1 samples before it
                c16 = np.round(c * 16).astype(np.int64)
                s16 = np.round(e["local_sum"] * 16).astype(np.int64) - c16
                D = (1 << c_shift(W)) - 1
                tie = e["metric_valid"] & (c16 * D == s16)
                assert np.array_equal(tie, e["metric_valid"] & (e["corr_scaled"] == e["thresh_scaled"]))
                if (tie & ab).any():
                    got.add("cfar_tie_above")
                if (e["metric_valid"] & ((c16 + 1) * D == s16) & ~ab).any():
                    got.add("cfar_under_tie")
                if (~ab & e["gate_mask"] & (c >= 4 / 16.0)).any():
                    got.add("large_non_above_in_gate")
            elif (ab & (c == 0.5)).any():
                got.add("min_tie_above")
    return got


def required(n, W, hyst):
    """{fact: arithmetic predicate on (n, W, Hp) under which the streams must hold it}.  Each predicate is
    what the construction in family_m / family_c needs to fit inside [W, n); none fails at (1024, 128, 64)
    or (1024, 128, 256)."""
    Hp = max(hyst, 1)
    room = n - W                                               # valid samples
    D = (1 << c_shift(W)) - 1
    pow2 = W >= 128 and W == 2 * (D + 1)
    return {
        "silent": True,
        "all_above": room >= 1,
        "pre_valid_ignored": room >= 1,
        "first_valid_above": room >= 1,
        "min_tie_above": room >= 8,                            # the 0.5 sample sits at W + 7
        # chain+0 places W, W + Hp - 1, W + 2 Hp - 1, W + 3 Hp: all three gaps need W + 3 Hp <= n - 1
        "gap_Hp-1": Hp >= 2 and W + 3 * Hp <= n - 1,
        "gap_Hp+0": W + 3 * Hp <= n - 1,
        "gap_Hp+1": W + 3 * Hp <= n - 1,
        # a lone pulse at p in [W + 1, W + 128] closes at p + Hp: every residue mod 128 fits when
        # W + 128 + Hp <= n - 1
        "end%64=0": W + 128 + Hp <= n - 1, "end%64=63": W + 128 + Hp <= n - 1,
        "end%128=0": W + 128 + Hp <= n - 1, "end%128=127": W + 128 + Hp <= n - 1,
        "start%64=0": W + 128 <= n - 1, "start%64=63": W + 128 <= n - 1,
        "start%128=0": W + 128 <= n - 1, "start%128=127": W + 128 <= n - 1,
        # close at p + Hp, reopen at p + Hp + 1, p <= W + 128
        "reopen_same_row": W + 128 + Hp + 1 <= n - 1,
        "reopen_next_row": W + 128 + Hp + 1 <= n - 1,
        "reopen_next_chunk": W + 128 + Hp + 1 <= n - 1,
        # min_chain closes at W + Hp + k (Hp + 1): two in one chunk need Hp + 1 <= 64 and three closes in range
        "two_closes_in_chunk": Hp <= 64 and W + 4 * (Hp + 1) <= n - 1,
        "more_than_8_events": W + 9 * (Hp + 1) <= n,
        "close_on_last_sample": n - 1 - Hp >= W,
        "open_end_close_at_n": n - Hp >= W,
        "open_end_close_at_n+1": n + 1 - Hp >= W and Hp >= 2,   # Hp = 1: the sample is n itself
        "above_at_n-1": room >= 1,
        # the block of above samples from W + 3 holds 2.0 at +5, +69 and +133, and at +0 and +130
        "tie_other_row": W + 3 + 5 + 64 <= n - 1,
        "tie_other_chunk": W + 3 + 5 + 128 <= n - 1,
        "tie_with_opener": room >= 2,
        "cfar_tie_above": room >= 1,
        "cfar_under_tie": room >= 1,
        # family C gates open at i = W with a tie at 14 / 16 on a window shaped before it; the sum must then
        # rise by D + 1 within the gate through non-above samples of 13 / 16 replacing ones, D / 12 + 2
        # samples: 7, 12 and 44 for the power-of-two windows 128, 256 and 1024, fewer than the 63 non-above
        # samples a fused gate survives.  Other windows and shorter hysteresis are not required to hold it.
        "large_non_above_in_gate": pow2 and D // 12 + 3 <= min(Hp, 64) - 1 and W + D // 12 + 3 <= n - 1,
        "peak_non_above": pow2 and D // 12 + 3 <= min(Hp, 64) - 1 and W + D // 12 + 3 <= n - 1,
        "peak_on_close": pow2 and D // 12 + 3 <= min(Hp, 64) - 1 and W + Hp <= n - 1,
    }


def check(n, W, hyst):
    """Exactness against int64 arithmetic, the batch size, and every required fact present; returns the
    facts found."""
    st, exp = streams(n, W, hyst), expected(n, W, hyst)
    assert sum(len(bt.names) for bt in st.values()) >= MIN_STREAMS
    for k, bt in st.items():
        assert bt.c.shape == (len(bt.names), n) and len(set(bt.names)) == len(bt.names)
        _exact(bt, exp[k], hyst)
    got = facts(n, W, hyst)
    req = required(n, W, hyst)
    if (n, W, hyst) in ((1024, 128, 64), (1024, 128, 256)):
        # nothing is waived at these two; the two facts of the minimal chain exist at Hp = 64 only
        waived = [k for k, v in req.items() if not v and not (k in ("two_closes_in_chunk", "more_than_8_events")
                                                               and hyst == 256)]
        assert not waived, waived
    missing = sorted(k for k, v in req.items() if v and k not in got)
    assert not missing, (n, W, hyst, missing)
    return got
