"""Exact metric streams for the detection post-processing (csrc/postproc.hip: trailing_avg_kernel,
plateau_kernel, minn_peak_kernel, sc_gate_kernel, segment_peak_kernel).

NumPy and the CPU oracle only.  Metric values are multiples of 2^-4 in [0, 1] and the smoothing windows
are powers of two (1, 4, 8, 16), so every window sum and every sum * (1 / w) is exact in any order: the
kernel's ascending-order smoothed metric equals np.convolve's bit for bit (ms_ascending, checked for every
stream), float32 holds the same values, and ties are real.  Three kinds of stream leave the grid on
purpose: the level families put a sample on exactly the double 0.95 * max or 0.6 * peak (w = 1, so Ms is
M), the S&C gate family takes negative sixteenths, and the non-finite family holds NaN and +-inf.
Expected results always come from ofdm_oracle (expected()), never from the pattern a stream was built
from; a ValueError of the oracle is the status code the kernels report (-1, -2, -3).

A Case is one launch: an entry point (op), one parameter set and all streams of a family at one length.
  op       params                      data            result per stream
  plateau  (cp, lookahead, w)          M               (index, status = branch or -3, Ms)
  minn     (w, thr, bounds)            M               (peak, gate_lo, gate_hi, status, Ms)
  trail    (win, clip)                 x               (y,)
  gate     (thr,)                      M               (mask, first, last + 1)
  seg      (bounds,)                   Ms, mask        (peak, status)
  detect   (w, thr, bounds)            M_minn, M_sc    (peak, status, first, last + 1)
cases(n) lists them, expected(n, f32) holds the oracle's results, check(n) asserts the preconditions and
that every fact required(n) asks for is present, and MUTANTS are single wrong decisions of the oracle's
functions (run(..., mut)), each of which must change the result of a stream (mutants_caught).
"""
import functools
from collections import namedtuple

import numpy as np

import ofdm_oracle as O

NS = (1, 2, 7, 8, 9, 255, 256, 257, 511, 513, 1025)
WS = (1, 4, 8, 16)
CPS = (0, 1, 8, 16, 64)
PW = 256                                   # threads per stream in postproc.hip
THR_MUL = float(np.nextafter(1.0 / 3.0, 1.0))   # (1/16) / (3/16) < THR_MUL, yet 1/16 >= THR_MUL * (3/16) in float64
GATE_THRS = (0.6, 1.5, -0.25, THR_MUL)
MINN_THRS = (0.5, 0.75)
NAN, INF = float("nan"), float("inf")

Case = namedtuple("Case", "op family n params names data")


def chunk(length):
    """C of for_each_run: thread t owns [t * C, (t + 1) * C) of a range of `length`."""
    return max(1, -(-length // PW))


def lookaheads(n):
    """None, a small one, and one beyond the metric so that hi = Lo - L - 1 is negative and wraps."""
    return (None, 3, n + 2)


def bounds_set(n):
    """None, a window that cuts, the last two samples, and start >= end (the whole range)."""
    return (None, (n // 4, n // 2), (n - 2, n), (n // 2, n // 4))


# ------------------------------------------------------------------------------------------
# stream pools (values in sixteenths)
# ------------------------------------------------------------------------------------------
def _g(n, k=2):
    return np.full(n, k / 16.0)


def _put(c, pairs):
    for i, k in pairs:
        if 0 <= i < c.size:
            c[i] = k / 16.0
    return c


def _blk(a, b, k):
    return [(i, k) for i in range(a, b)]


def pool_ties(n):
    out = [("zeros", np.zeros(n)), ("flat", _g(n, 8))]
    a = n // 4
    out.append(("plateau", _put(_g(n), _blk(a, a + max(1, n // 3), 12))))
    # two equal maxima whose distance is decided by lanes (< 64), waves (64..255), the stride (>= 256)
    for d in (1, 63, 64, 255, 256, 300, 512):
        if 5 + d < n:
            out.append((f"tie+{d}", _put(_g(n), [(5, 14), (5 + d, 14)])))
    out.append(("tie_ends", _put(_g(n), [(0, 14), (n - 1, 14)])))
    up = np.minimum(16, np.arange(n) * 17 // n) / 16.0
    out += [("ramp_up", up), ("ramp_down", up[::-1].copy()), ("peak_last", _put(_g(n, 8), [(n - 1, 16)])),
            ("saw", (np.arange(n) % 17) / 16.0), ("saw_down", (16 - np.arange(n) % 17) / 16.0)]
    return out


def run_span(n):
    return max(10 * chunk(n), 70) if n >= 255 else max(1, n // 2)


def pool_runs(n):
    """Two-level streams (16 / 2 sixteenths): runs whose first and last sample lie on, one before and one
    after a multiple of C, long enough to span many per-thread chunks and to outlast cp = 64."""
    C, sp = chunk(n), run_span(n)
    out = []
    for ds in (-1, 0, 1):
        for de in (-1, 0, 1):
            s, e = 3 * C + ds, (3 + -(-sp // C)) * C + de
            if 0 <= s < e <= n:
                out.append((f"run{ds:+d}{de:+d}", _put(_g(n), _blk(s, e, 16))))
    s = 3 * C
    out.append(("two_runs", _put(_g(n), _blk(s, s + sp, 16) + _blk(s + sp + 5, s + 2 * sp + 6, 16))))
    out.append(("short_long", _put(_g(n), _blk(C, C + 3, 16) + _blk(C + 7, C + 7 + sp, 16))))
    out.append(("run_to_end", _put(_g(n), _blk(n - sp, n, 16))))
    out.append(("all_hi", _g(n, 16)))
    out.append(("singles", _put(_g(n), [(k, 16) for k in range(0, n, 7 * C)])))
    return out


def pool_rand(n):
    rng = np.random.default_rng(1000 + n)
    out = []
    for j in range(4):
        out.append((f"u{j}", rng.integers(0, 17, n) / 16.0))
    for j in range(4):                                           # sparse: zeros with a few blocks
        c = np.zeros(n)
        for _ in range(3):
            s, ln = int(rng.integers(0, n)), int(rng.integers(1, 40))
            c[s:s + ln] = int(rng.integers(1, 17)) / 16.0
        out.append((f"sp{j}", c))
    for j in range(4):                                           # piecewise constant on three levels
        c, i = np.empty(n), 0
        while i < n:
            ln = int(rng.geometric(1.0 / (4 + 8 * j)))
            c[i:i + ln] = (4, 10, 16)[int(rng.integers(0, 3))] / 16.0
            i += ln
        out.append((f"lv{j}", c))
    return out


def pool_metric(n):
    return pool_ties(n) + pool_runs(n) + pool_rand(n)


def pool_nonfinite(n):
    rng = np.random.default_rng(2000 + n)
    base = rng.integers(1, 17, n) / 16.0
    mid = n // 2

    def w(pairs, c=base):
        c = c.copy()
        for i, v in pairs:
            if 0 <= i < n:
                c[i] = v
        return c

    out = [("all_nan", np.full(n, NAN)), ("nan_first", w([(0, NAN)])), ("nan_mid", w([(mid, NAN)])),
           ("nan_last", w([(n - 1, NAN)])), ("all_ninf", np.full(n, -INF)), ("pinf_mid", w([(mid, INF)])),
           ("pinf_first", w([(0, INF)])), ("pinf_last", w([(n - 1, INF)])), ("ninf_mid", w([(mid, -INF)])),
           ("inf_pair", w([(mid, INF), (mid + 1, -INF)])), ("two_pinf", w([(mid, INF), (mid + 3, INF)])),
           ("nan_then_pinf", w([(mid, NAN), (mid + 2, INF)])), ("pinf_then_nan", w([(mid, INF), (mid + 2, NAN)])),
           ("two_nan", w([(n // 3, NAN), (mid + 1, NAN)]))]
    step = np.where(np.arange(n) < n // 3, 0.5, 1.0)             # 0.5 ... NaN 1.0 ...: the unnormalised gate
    out.append(("half_nan_one", w([(n // 3, NAN)], step)))
    out.append(("flat_ninf_mid", w([(mid, -INF)], _g(n, 8))))
    out.append(("neg_nan", w([(mid, NAN)], -base)))
    return out


def fam_p95(n, cp):
    """w = 1: a sample on exactly the double 0.95 * m at center + cp - 1 (inside the window: <= holds,
    < does not) or at center + cp (outside)."""
    out = []
    for mk in (16, 12, 11):
        m = mk / 16.0
        for p in (0, 3):
            if cp < 2 or p + cp + 1 > n:
                continue
            base = np.full(n, m)
            base[:p] = 1 / 16.0
            for tag, at in (("in", p + cp - 1), ("out", p + cp)):
                c = base.copy()
                c[at] = 0.95 * m
                out.append((f"p95_{tag}_m{mk}_p{p}", c))
    return out


def fam_p60(n, cp):
    """w = 1: the maximum m on the last sample (so the 95 % branch is skipped) and runs of samples on
    exactly the double 0.6 * m: of min_run, of min_run - 1, short then long, two long, one up to the end."""
    mr = max(8, cp // 2)
    out = []
    for mk in (16, 12, 11):                                      # 0.6 * m is off the grid for these
        m = mk / 16.0
        lv = 0.6 * m

        def mk_stream(runs, name):
            if max(e for _, e in runs) > n - 1 and name != "to_end":
                return
            c = np.zeros(n)
            for s, e in runs:
                c[s:e] = lv
            c[n - 1] = m
            out.append((f"p60_{name}_m{mk}", c))

        if n < mr + 3:
            continue
        mk_stream([(2, 2 + mr)], "exact")
        mk_stream([(2, 1 + mr)], "short")
        mk_stream([(2, 1 + mr), (3 + mr, 5 + 2 * mr)], "short_long")
        mk_stream([(2, 2 + mr), (4 + mr, 4 + 2 * mr)], "two")
        mk_stream([(n - mr, n)], "to_end")
        mk_stream([(n - mr + 1, n)], "to_end_short")
    return out


def fam_mgate(n):
    """minn peak: gate threshold 0.5 and a maximum of 1, so samples of 8 / 16 sit exactly on thr * max."""
    a, b = n // 4, n // 2
    L = max(2, n // 16)
    out = []

    def add(name, pairs, base=0):
        out.append((name, _put(_g(n, base), pairs)))

    # two longest runs of equal length, the maximum in the later one: the earlier run is the gate
    add("two_equal_runs", _blk(2, 2 + L, 8) + _blk(4 + L, 4 + 2 * L, 8) + [(5 + L, 16)])
    add("later_longer", _blk(2, 2 + L, 8) + _blk(4 + L, 5 + 2 * L, 8) + [(5 + L, 16)])
    add("earlier_longer", _blk(2, 3 + L, 8) + _blk(5 + L, 5 + 2 * L, 8) + [(6 + L, 16)])
    add("level_edge", _blk(2, 2 + L, 8) + [(1, 7), (2 + L, 7), (3, 16)])
    add("tied_peak", _blk(2, 2 + L, 8) + [(3, 16), (2 + L - 1, 16)])
    # bounds (n // 4, n // 2) cut this gate at both ends; the maximum lies outside them
    add("cut_both", _blk(a - 3, b + 3, 8) + [(a - 2, 16), (a + 1, 12), (b - 1, 12)])
    add("starts_at_lo", _blk(a, b, 8) + [(a, 16)])
    add("bounds_miss", _blk(b + 2, b + 2 + L, 8) + [(b + 3, 16)])
    add("gate_is_last", _blk(n - 3, n, 8) + [(n - 1, 16)])
    # two longest runs of one sample each that start in ONE per-thread chunk of for_each_run (C >= 3):
    # the thread itself has to keep the earlier one before the block reduction sees either
    q = 10 * chunk(n)
    add("pair_in_chunk", [(q, 16), (q + 2, 16)], 2)
    add("pairs_in_chunks", [(q, 16), (q + 2, 16), (2 * q, 16), (2 * q + 2, 16)], 2)
    add("all_neg", [(i, -(1 + i % 5)) for i in range(n)])
    add("one_positive", [(i, -3) for i in range(n)] + [(n // 3, 1)])
    return out


def fam_gate(n):
    """S&C gate: (v, max) = (3, 5), (6, 10), (9, 15) sixteenths have the quotient 0.6 exactly; (1, 3), (2, 6)
    and (4, 12) separate M / max >= THR_MUL from M >= THR_MUL * max."""
    out = []
    for v, m in ((3, 5), (6, 10), (9, 15), (1, 3), (2, 6), (4, 12)):
        out.append((f"pair_{v}_{m}", _put(_g(n, 0), [(4, m), (6, v - 1), (2, v), (n - 1, v)] if n > 6 else
                                           [(0, m), (n - 1, v)] if n > 1 else [(0, m)])))
        out.append((f"pair_{v}_{m}_inner", _put(_g(n, 0), [(n // 2, m), (n // 3, v), (n // 2 + 1, v - 1)])))
    out.append(("neg", _put(_g(n), [(i, -(1 + i % 5)) for i in range(n)])))
    out.append(("neg_flat", _g(n, -4)))
    out.append(("neg_tie_ends", _put(_g(n, -9), [(0, -3), (n - 1, -3)])))
    out.append(("max0", _put(_g(n, 0), [(i, -2) for i in range(0, n, 3)])))
    return out


def fam_seg(n):
    """(name, Ms, mask) for the first-run peak with bounds None or (n // 4, n // 2)."""
    rng = np.random.default_rng(3000 + n)
    a, b = n // 4, n // 2
    out = []

    def add(name, runs, pairs, base=None):
        mask = np.zeros(n, bool)
        for s, e in runs:
            mask[max(0, s):max(0, e)] = True
        out.append((name, _put(_g(n, 1) if base is None else base.copy(), pairs), mask))

    u = rng.integers(0, 17, n) / 16.0
    add("second_higher", [(2, 6), (8, 12)], [(3, 9), (9, 15)])
    add("equal_later", [(1, n - 1)], [(2, 12), (n - 3, 12)])
    add("equal_to_seed", [(1, n - 1)], [(1, 12), (4, 12)])
    add("first_short_then_long", [(a, a + 2), (a + 4, b)], [(a + 1, 5), (a + 6, 16)])
    add("cut_hi", [(b - 4, b + 4)], [(b - 2, 8), (b + 2, 16)])
    add("starts_at_lo", [(a, a + 5)], [(a, 9), (a + 2, 9)])
    add("starts_before_lo", [(a - 3, a + 5)], [(a - 2, 16), (a + 3, 8)])
    add("run_outside", [(b + 1, b + 4)], [(b + 2, 16)])
    add("all_true", [(0, n)], [], u)
    add("all_false", [], [], u)
    add("last_only", [(n - 1, n)], [], u)
    for j, lv in enumerate((4, 10, 14)):
        out.append((f"rand_mask{j}", u, rng.integers(0, 17, n) >= lv))
    C, sp = chunk(n), run_span(n)
    for ds, de in ((-1, 1), (0, 0), (1, -1)):
        add(f"run{ds:+d}{de:+d}", [(3 * C + ds, 3 * C + sp + de)], [], u)
    return out


def fam_seg_nonfinite(n):
    rng = np.random.default_rng(4000 + n)
    u = rng.integers(1, 16, n) / 16.0                            # below 1.0, the maximum placed by hand
    out = []

    def add(name, run, vals, base=u):
        mask = np.zeros(n, bool)
        mask[max(0, run[0]):max(0, run[1])] = True
        c = base.copy()
        for i, v in vals:
            if 0 <= i < n:
                c[i] = v
        out.append((name, c, mask))

    s, e = n // 4, n // 4 + max(2, n // 3)
    add("nan_at_start", (s, e), [(s, NAN)])
    add("nan_later", (s, e), [(s + 1, NAN)])
    add("nan_before_max", (s, e), [(s + 1, NAN), (e - 1, 1.0)])
    add("nan_after_max", (s, e), [(s, 1.0), (e - 1, NAN)])
    add("nan_before_run", (s + 1, e), [(s, NAN)])
    add("ninf_run", (s, e), [], np.full(n, -INF))
    add("ninf_seed", (s, e), [(s, -INF)])
    add("pinf_twice", (s, e), [(s + 1, INF), (e - 1, INF)])
    add("all_nan", (0, n), [], np.full(n, NAN))
    add("all_nan_no_mask", (0, 0), [], np.full(n, NAN))
    return out


# ------------------------------------------------------------------------------------------
# cases: one launch each
# ------------------------------------------------------------------------------------------
def _stack(rows, n):
    a = np.array([r for r in rows]).reshape(len(rows), n)
    a.setflags(write=False)
    return a


def _case(op, family, n, params, named, keys=("M",)):
    names = [t[0] for t in named]
    assert len(set(names)) == len(names), (family, names)
    data = {k: _stack([t[1 + j] for t in named], n) for j, k in enumerate(keys)}
    return Case(op, family, n, params, names, data)


@functools.lru_cache(maxsize=None)
def cases(n):
    """Every launch at length n; arrays are read-only (shared by every test)."""
    out = []
    metric, nonfin = pool_metric(n), pool_nonfinite(n)
    for fam, pool in (("metric", metric), ("nonfinite", nonfin)):
        for w in WS:
            for cp in CPS:
                for la in lookaheads(n):
                    out.append(_case("plateau", fam, n, (cp, la, w), pool))
            for thr in MINN_THRS:
                for bd in bounds_set(n):
                    out.append(_case("minn", fam, n, (w, thr, bd), pool))
            for clip in (1, 0):
                out.append(_case("trail", fam, n, (w, clip), pool, ("x",)))
        for thr in GATE_THRS:
            out.append(_case("gate", fam, n, (thr,), pool))
    for cp in CPS:
        for fam, rows in (("p95", fam_p95(n, cp)), ("p60", fam_p60(n, cp))):
            if rows:
                out.append(_case("plateau", fam, n, (cp, None, 1), rows))
    mg = fam_mgate(n)
    for w in WS:
        for bd in bounds_set(n):
            out.append(_case("minn", "mgate", n, (w, 0.5, bd), mg))
    for thr in GATE_THRS:
        out.append(_case("gate", "gate", n, (thr,), fam_gate(n)))
    for bd in bounds_set(n):
        out.append(_case("seg", "seg", n, (bd,), fam_seg(n), ("Ms", "mask")))
        out.append(_case("seg", "nonfinite", n, (bd,), fam_seg_nonfinite(n), ("Ms", "mask")))
    # the whole combined decision: S&C metric b gates Minn metric b + 7
    # and under an S&C metric that lets everything through: the Minn peak on the first and on the last
    # sample inside the bounds (n // 4, n // 2), and every non-finite Minn metric
    a, b, flat = n // 4, n // 2, _g(n, 8)
    edge = [("edge_hi|flat", _put(_g(n, 0), [(b - 1, 16), (b - 2, 12), (b, 16)]), flat),
            ("edge_lo|flat", _put(_g(n, 0), [(a, 16), (a + 1, 12), (a - 1, 16)]), flat)]
    for fam, pool, more in (("metric", metric + fam_gate(n) + mg, edge),
                            ("nonfinite", nonfin, [(f"{nm}|flat", c, flat) for nm, c in nonfin])):
        k = len(pool)
        pairs = [(f"{pool[(i + 7) % k][0]}|{pool[i][0]}", pool[(i + 7) % k][1], pool[i][1]) for i in range(k)]
        for w in (1, 16):
            for thr in (0.6, THR_MUL):
                for bd in bounds_set(n)[:2]:
                    out.append(_case("detect", fam, n, (w, thr, bd), pairs + more, ("M_minn", "M_sc")))
    return tuple(out)


def as_f32_values(a):
    """The float64 values a float32 copy of the stream holds (what a float32 launch computes on)."""
    return a.astype(np.float32).astype(np.float64) if a.dtype == np.float64 else a


# ------------------------------------------------------------------------------------------
# the oracle, and its mutants
# ------------------------------------------------------------------------------------------
def _smooth(M, w):
    return np.convolve(M, np.ones(w, dtype=float) / w, mode="same")          # sc.py:100


def oracle(op, params, row):
    """The result tuple of one stream from ofdm_oracle; row = the stream's arrays in the case's key order."""
    if op == "plateau":
        cp, la, w = params
        try:
            idx, br, Ms = O.plateau_end(row[0], cp, la, w)
        except ValueError:                                       # numpy's broadcast error: status -3
            idx, br, Ms = -1, -3, _smooth(row[0], max(1, w))
        return idx, br, Ms
    if op == "minn":
        w, thr, bd = params
        try:
            pk, gate, Ms = O.minn_peak(row[0], w, thr, bd)
        except ValueError:                                       # no positive peak: status -2
            return -1, 0, 0, -2, O.trailing_average(np.maximum(row[0], 0.0), max(1, w))
        idx = np.flatnonzero(gate)
        assert idx.size and idx[-1] - idx[0] + 1 == idx.size     # the gate is one run
        return pk, int(idx[0]), int(idx[-1]) + 1, 0, Ms
    if op == "trail":
        win, clip = params
        x = row[0]
        return (O.trailing_average(np.maximum(x, 0.0) if clip else x, win),)
    if op == "gate":
        mask, span = O.sc_gate(row[0], params[0])
        return mask, span[0], span[1]
    if op == "seg":
        Ms, mask = row
        lo, hi = O._bounds(Ms.size, params[0])
        m = mask.copy()
        m[:lo] = False
        m[hi:] = False
        if not m.any():                                          # combined_sc_min.py:245-246: status -1
            return -1, -1
        return int(O.streaming_peak(Ms, m)), 0
    if op == "detect":
        w, thr, bd = params
        mask, span = O.sc_gate(row[1], thr)
        try:
            return int(O.comb_minn_peak(row[0], w, mask, bd)), 0, span[0], span[1]
        except ValueError:
            return -1, -1, span[0], span[1]
    raise KeyError(op)


def _argmax(v, mut):
    if mut == "argmax_last":
        return v.size - 1 - int(np.argmax(v[::-1]))
    if mut == "nan_ignored":
        return 0 if np.isnan(v).all() else int(np.nanargmax(v))
    return int(np.argmax(v))


def _max(v, mut):
    if mut == "nan_ignored":
        return -INF if np.isnan(v).all() else float(np.nanmax(v))
    return float(np.max(v))


def _runs(mask, mut=None):
    runs = [(int(s), int(e)) for s, e in O._runs(mask)]
    if mut != "runs_split_C":
        return runs
    C, out = chunk(len(mask)), []
    for s, e in runs:
        cuts = [s] + list(range((s // C + 1) * C, e, C)) + [e]
        out += list(zip(cuts[:-1], cuts[1:]))
    return out


def _mbounds(n, bd, mut):
    lo, hi = O._bounds(n, bd)
    if bd is not None:
        lo += mut == "bounds_lo+1"
        hi -= mut == "bounds_hi-1"
    return lo, hi


def m_plateau(M, cp, la, w, mut):
    M = np.asarray(M, float)
    L = (cp // 4) if la is None else int(max(1, la))
    Ms = _smooth(M, max(1, w))
    center = _argmax(Ms, mut)
    post_hi = min(Ms.size, center + cp + {"post_hi-1": -1, "post_hi+1": 1}.get(mut, 0))
    if post_hi > center + 1:
        lv, seg = 0.95 * float(Ms[center]), Ms[center:post_hi]
        below = np.flatnonzero(seg < lv if mut == "p95_lt" else seg <= lv)
        if below.size:
            return int(center + below[0]), 1, Ms
    min_run = max(8, cp // 2) + {"min_run-1": -1, "min_run+1": 1}.get(mut, 0)
    peak = _max(Ms, mut)
    if peak > 0:
        lv = 0.6 * peak
        runs = [r for r in _runs(Ms > lv if mut == "p60_gt" else Ms >= lv, mut) if r[1] - r[0] >= min_run]
        if runs:
            s, e = runs[-1] if mut == "run_latest" else runs[0]
            return (e if mut == "run_e" else e - 1), 2, Ms
    lo, hi = max(0, center - cp), min(Ms.size - L - 1, center + cp)
    window, ahead = Ms[lo:hi], Ms[lo + L:hi + L]
    try:
        drop = window - ahead
    except ValueError:
        return -1, -3, Ms
    if drop.size == 0:
        return center, 4, Ms
    return lo + _argmax(drop, mut) + L // 2, 3, Ms


def m_minn(M, w, thr, bd, mut):
    M = np.asarray(M, float)
    Ms = O.trailing_average(np.maximum(M, 0.0), max(1, w))
    mx = _max(Ms, mut)
    if mx <= 0.0:
        return -1, 0, 0, -2, Ms
    lv = thr * mx
    best = None
    for s, e in _runs(Ms > lv if mut == "gate_gt" else Ms >= lv, mut):
        if best is None or e - s > best[1] - best[0] or (mut == "longest_tie_latest" and e - s == best[1] - best[0]):
            best = (s, e)
    if best is not None:
        lo, hi = _mbounds(M.size, bd, mut)
        s, e = max(best[0], lo), min(best[1], hi)
        if s < e:
            return s + _argmax(Ms[s:e], mut), s, e, 0, Ms
    pk = _argmax(Ms, mut)
    return pk, pk, pk + 1, 0, Ms


def m_gate(M, thr, mut):
    M = np.asarray(M, float)
    mx = _max(M, mut)
    with np.errstate(all="ignore"):
        q, t = (M, thr * mx) if mut == "gate_mul" else (M / mx, thr)
        if not mx > 0:
            q, t = M, thr
        mask = q > t if mut == "gate_thr_gt" else q >= t
    if not mask.any():
        mask = np.zeros(M.size, bool)
        mask[_argmax(M, mut)] = True
    idx = np.flatnonzero(mask)
    return mask, int(idx[0]), int(idx[-1]) + (mut != "span_last")


def m_seg(Ms, mask, bd, mut):
    lo, hi = _mbounds(Ms.size, bd, mut)
    m = np.asarray(mask, bool).copy()
    m[:lo] = False
    m[hi:] = False
    runs = _runs(m)
    if not runs:
        return -1, -1
    s, e = runs[0]
    if mut == "seg_last_run":
        s, e = runs[-1]
    if mut == "seg_longest_run":
        s, e = max(runs, key=lambda r: (r[1] - r[0], -r[0]))
    if mut == "seg_nan_max":
        return s + int(np.argmax(Ms[s:e])), 0
    best, bi = Ms[s], s
    for i in range(s + 1, e):
        if (Ms[i] >= best) if mut == "seg_ge" else (Ms[i] > best):
            best, bi = Ms[i], i
    return bi, 0


def run(op, params, row, mut=None):
    """The oracle's functions restated with one deliberate error `mut`; without one the result equals
    oracle(), which check() asserts for every stream."""
    with np.errstate(all="ignore"):
        if op == "plateau":
            return m_plateau(row[0], *params, mut)
        if op == "minn":
            return m_minn(row[0], *params, mut)
        if op == "trail":
            return oracle(op, params, row)
        if op == "gate":
            return m_gate(row[0], params[0], mut)
        if op == "seg":
            return m_seg(row[0], row[1], params[0], mut)
        w, thr, bd = params
        mask, first, last1 = m_gate(row[1], thr, mut)
        Ms = O.trailing_average(np.maximum(np.asarray(row[0], float), 0.0), max(1, w))
        return m_seg(Ms, mask, bd, mut) + (first, last1)


# mutant -> the ops whose result it can change
MUTANTS = {
    "argmax_last": ("plateau", "minn", "gate"),
    "p95_lt": ("plateau",),
    "p60_gt": ("plateau",),
    "gate_gt": ("minn",),
    "gate_thr_gt": ("gate", "detect"),
    "post_hi-1": ("plateau",),
    "post_hi+1": ("plateau",),
    "min_run-1": ("plateau",),
    "min_run+1": ("plateau",),
    "run_latest": ("plateau",),
    "run_e": ("plateau",),
    "runs_split_C": ("plateau", "minn"),
    "longest_tie_latest": ("minn",),
    "bounds_lo+1": ("minn", "seg", "detect"),
    "bounds_hi-1": ("minn", "seg", "detect"),
    "gate_mul": ("gate", "detect"),
    "span_last": ("gate", "detect"),
    "seg_last_run": ("seg", "detect"),
    "seg_longest_run": ("seg", "detect"),
    "seg_ge": ("seg", "detect"),
    "nan_ignored": ("plateau", "minn", "gate"),
    "seg_nan_max": ("seg", "detect"),
}
MUTANT_NS = (257, 1025)                    # runs_split_C needs C > 1


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def rows(case, f32=False):
    keys = list(case.data)
    arrs = [as_f32_values(case.data[k]) if f32 else case.data[k] for k in keys]
    return [[a[b] for a in arrs] for b in range(len(case.names))]


@functools.lru_cache(maxsize=None)
def expected(n, f32=False):
    """Per case of cases(n), the oracle's result tuple of every stream (on the float32 values for f32)."""
    out = []
    with np.errstate(all="ignore"):
        for j, c in enumerate(cases(n)):
            if f32 and all(np.array_equal(as_f32_values(a), a, equal_nan=True) for a in c.data.values()):
                out.append(expected(n)[j])                       # float32 holds the same values
            else:
                out.append([oracle(c.op, c.params, r) for r in rows(c, f32)])
    return tuple(out)


NAN_MUTANTS = ("nan_ignored", "seg_nan_max")  # judged on the non-finite family, every other one on finite streams
# (mutant, op, family): the family built for that decision has to catch it too, not only a chance stream
TARGETS = (
    ("p95_lt", "plateau", "p95"), ("post_hi-1", "plateau", "p95"), ("post_hi+1", "plateau", "p95"),
    ("p60_gt", "plateau", "p60"), ("min_run-1", "plateau", "p60"), ("min_run+1", "plateau", "p60"),
    ("run_latest", "plateau", "p60"), ("run_e", "plateau", "p60"),
    ("gate_gt", "minn", "mgate"), ("longest_tie_latest", "minn", "mgate"), ("argmax_last", "minn", "mgate"),
    ("bounds_lo+1", "minn", "mgate"), ("bounds_hi-1", "minn", "mgate"),
    ("gate_thr_gt", "gate", "gate"), ("gate_mul", "gate", "gate"), ("argmax_last", "gate", "gate"),
)


def _first_catch(mut, op, family, ns):
    for n in ns:
        for c, exp in zip(cases(n), expected(n)):
            if c.op != op or (c.family != family if family else (c.family == "nonfinite") != (mut in NAN_MUTANTS)):
                continue
            hit = [(n, c.family, c.params, c.names[b]) for b, r in enumerate(rows(c))
                   if not same(run(c.op, c.params, r, mut), exp[b])]
            if hit:
                return hit
    return []


def mutants_caught(ns=MUTANT_NS):
    """{(mutant, op, family or None): [(n, family, params, stream)] on which it changes the oracle's
    result}: the streams of the first case that catches it, searched over ns in order.  With family None
    a mutant of a finite decision is judged on the finite families only, the NaN mutants on the
    non-finite one; the TARGETS are judged on their own family."""
    out = {(mut, op, None): _first_catch(mut, op, None, ns) for mut, ops in MUTANTS.items() for op in ops}
    out.update({t: _first_catch(*t, ns) for t in TARGETS})
    return out


# ------------------------------------------------------------------------------------------
# check(): preconditions and coverage
# ------------------------------------------------------------------------------------------
def ms_ascending(M, w, descending=False):
    """The kernel's smoothed metric: Lo = max(n, w) outputs, Ms[i] = sum over j ascending in
    [i + off - w + 1, i + off] ∩ [0, n) of M[j] * (1 / w), off = (min(n, w) - 1) // 2."""
    n = M.size
    Lo, off, vw = max(n, w), (min(n, w) - 1) // 2, 1.0 / w
    Ms, i = np.zeros(Lo), np.arange(Lo)
    with np.errstate(all="ignore"):
        for k in (range(w - 1, -1, -1) if descending else range(w)):   # the k-th term of every window
            j = i + off - w + 1 + k
            ok = (j >= 0) & (j < n)
            Ms[ok] = Ms[ok] + M[j[ok]] * vw
    return Ms


def on_grid(a):
    f = a[np.isfinite(a)] * 16.0
    return bool(np.all(f == np.round(f)) and np.all(np.abs(f) <= 16))


def _preconditions(n):
    seen = set()
    for c, exp in zip(cases(n), expected(n)):
        for k, a in c.data.items():
            assert a.shape == (len(c.names), n), (c.family, k)
            if a.dtype == bool:
                continue
            if c.family in ("p95", "p60"):
                cp, la, w = c.params
                assert w == 1                                    # Ms is M: the level samples stay exact
                f = 0.95 if c.family == "p95" else 0.6
                for b in range(len(c.names)):
                    m = a[b].max()
                    off = a[b][~np.isin(a[b] * 16.0, np.arange(17.0))]
                    assert m * 16 in np.arange(17.0) and off.size and np.all(off == f * m), c.names[b]
            else:
                assert on_grid(a), (c.family, c.op, k)
                if c.family != "nonfinite":
                    assert np.isfinite(a).all() and np.array_equal(as_f32_values(a), a)
        for b, r in enumerate(rows(c)):
            assert same(run(c.op, c.params, r), exp[b]), (c.op, c.family, c.params, c.names[b])
        if c.op == "plateau":
            w = c.params[2]
            for b, name in enumerate(c.names):
                key = (c.family, name, w)
                if key not in seen:                              # Ms depends on the stream and w only
                    seen.add(key)
                    assert np.array_equal(exp[b][2], ms_ascending(c.data["M"][b], w), equal_nan=True), key


def facts(n):
    """{family group: set of coverage facts present in the oracle's output at length n}."""
    got = {k: set() for k in ("plateau", "minn", "gate", "seg", "nonfinite")}
    for c, exp in zip(cases(n), expected(n)):
        nf = c.family == "nonfinite"
        for b, name in enumerate(c.names):
            e = exp[b]
            if c.op == "plateau":
                g = got["nonfinite" if nf else "plateau"]
                cp, la, w = c.params
                M, (idx, br, Ms) = c.data["M"][b], e
                Lo, C = Ms.size, chunk(Ms.size)
                if nf:
                    if np.isnan(M).all():
                        g.add("pl_all_nan")
                    if (M == -INF).all():
                        g.add("pl_all_ninf")
                    if np.isnan(Ms).any() and not np.isnan(M).any():
                        g.add("pl_ms_nan_from_inf")
                    if np.isnan(Ms).any() and br in (3, 4, -3):
                        g.add(f"pl_nan_branch{br}")
                    if np.isnan(Ms).any() and not np.isnan(Ms).all() and not np.isnan(Ms[0]) and br == 3:
                        g.add("pl_partial_nan_fallback")
                    continue
                g.add({0: "pl_empty", 1: "pl_branch1", 2: "pl_branch2", 3: "pl_branch3", 4: "pl_branch4",
                       -3: "pl_raise"}[br])
                if n < w:
                    g.add("pl_n<w")
                center = int(np.argmax(Ms))
                at = np.flatnonzero(Ms == Ms[center])
                for d in at[1:] - center:
                    g.add("pl_center_tie_d<64" if d < 64 else "pl_center_tie_64<=d<256" if d < 256 else
                          "pl_center_tie_d>=256")
                    if d == 256:
                        g.add("pl_center_tie_same_thread")
                if cp > 1 and center == Lo - 1:
                    g.add("pl_center_last_skips_95")
                lv95 = 0.95 * Ms[center]
                if br == 1 and Ms[idx] == lv95 and idx == center + cp - 1:
                    g.add("pl_95_equal_last_in_window")
                if br != 1 and center + cp < Lo and Ms[center + cp] == lv95:
                    g.add("pl_95_equal_first_outside")
                if br == 2:
                    mr, lv = max(8, cp // 2), 0.6 * Ms[center]
                    rr = _runs(Ms >= lv)
                    ok = [r for r in rr if r[1] - r[0] >= mr]
                    s, e_ = ok[0]
                    assert e_ - 1 == idx
                    if (Ms[s:e_] == lv).any():
                        g.add("pl_60_equal_in_run")
                    if e_ - s == mr:
                        g.add("pl_run_equals_min_run")
                    if any(r[1] - r[0] == mr - 1 for r in rr if r[0] < s):
                        g.add("pl_short_run_before")
                    if len(ok) > 1:
                        g.add("pl_two_long_runs")
                    if e_ == Lo:
                        g.add("pl_run_to_end")
                    if e_ - s >= 3 * C:
                        for tag, v in (("start", s), ("end", e_)):
                            for res, nm in ((0, "0"), (1, "1"), (C - 1, "C-1")):
                                if v % C == res:
                                    g.add(f"pl_run_{tag}%C={nm}")
                elif Ms[center] > 0 and any(r[1] - r[0] == max(8, cp // 2) - 1 for r in _runs(Ms >= 0.6 * Ms[center])):
                    g.add("pl_only_short_run")
                if br in (3, 4, -3):
                    L = (cp // 4) if la is None else max(1, la)
                    lo, hi = max(0, center - cp), min(Lo - L - 1, center + cp)
                    if hi < 0:
                        g.add("pl_slice_wraps")
                    if br == 3:
                        drop = Ms[lo:hi] - Ms[lo + L:hi + L]
                        if (drop == drop.max()).sum() > 1:
                            g.add("pl_drop_tie")
            elif c.op == "minn":
                g = got["nonfinite" if nf else "minn"]
                w, thr, bd = c.params
                pk, glo, ghi, st, Ms = e
                if nf:
                    if np.isnan(Ms).any() and st == 0 and ghi == glo + 1 and np.isnan(Ms[pk]):
                        g.add("mn_nan_is_peak")
                    if st == -2 and (c.data["M"][b] == -INF).all():
                        g.add("mn_all_ninf_status-2")
                    if st == 0 and Ms[pk] == INF:
                        g.add("mn_pinf_peak")
                    continue
                g.add(f"mn_status{st}")
                if st != 0:
                    continue
                C = chunk(n)
                lv = thr * Ms.max()
                rr = _runs(Ms >= lv)
                ln = max(r[1] - r[0] for r in rr)
                longest = [r for r in rr if r[1] - r[0] == ln]
                s, e_ = longest[0]
                if len(longest) > 1:
                    g.add("mn_longest_tie")
                    if longest[0][0] // C == longest[1][0] // C:
                        g.add("mn_longest_tie_in_one_chunk")
                if (Ms[s:e_] == lv).any():
                    g.add("mn_level_equal_in_gate")
                lo, hi = O._bounds(n, bd)
                if bd is not None and lo > s and hi < e_ and lo < hi:
                    g.add("mn_bounds_cut_both_ends")
                if max(s, lo) >= min(e_, hi):
                    g.add("mn_bounds_remove_gate")
                    assert pk == int(np.argmax(Ms)) and (glo, ghi) == (pk, pk + 1)
                elif (Ms[glo:ghi] == Ms[pk]).sum() > 1:
                    g.add("mn_peak_tie_in_gate")
                if ln >= 3 * C:
                    for tag, v in (("start", s), ("end", e_)):
                        for res, nm in ((0, "0"), (1, "1"), (C - 1, "C-1")):
                            if v % C == res:
                                g.add(f"mn_run_{tag}%C={nm}")
            elif c.op == "gate":
                g = got["nonfinite" if nf else "gate"]
                thr = c.params[0]
                M, (mask, first, last1) = c.data["M"][b], e
                if nf:
                    if np.isnan(M).all() or (M == -INF).all():
                        assert (first, last1) == (0, 1)
                        g.add("gt_all_nan_or_ninf_seed0")
                    elif np.isnan(M).any():
                        g.add("gt_nan_unnormalised" if (M[~np.isnan(M)] >= thr).any() else "gt_nan_seeded")
                    continue
                mx = M.max()
                with np.errstate(all="ignore"):
                    if mx > 0:
                        if (M / mx == thr).any():
                            g.add("gt_quotient_equal")
                        if ((M / mx >= thr) != (M >= thr * mx)).any():
                            g.add("gt_divide_differs_from_multiply")
                        if (M + 1 / 16.0 == thr * mx).any() or ((M + 1 / 16.0) / mx == thr).any():
                            g.add("gt_one_sixteenth_below")
                    g.add("gt_max>0" if mx > 0 else "gt_max=0" if mx == 0 else "gt_max<0")
                    passed = (M / mx >= thr) if mx > 0 else (M >= thr)
                if not passed.any():
                    g.add("gt_seeded_by_argmax")
                    if (M == mx).sum() > 1:
                        g.add("gt_seed_tie")
                if last1 == n and mask.sum() > 1:
                    g.add("gt_span_to_last")
            elif c.op == "seg":
                g = got["nonfinite" if nf else "seg"]
                Ms, mask = c.data["Ms"][b], c.data["mask"][b]
                pk, st = e
                lo, hi = O._bounds(n, c.params[0])
                m = mask.copy()
                m[:lo] = False
                m[hi:] = False
                rr = _runs(m)
                if st == -1:
                    g.add("sg_empty_status-1")
                    continue
                s, e_ = rr[0]
                if nf:
                    if np.isnan(Ms[s]):
                        assert pk == s
                        g.add("sg_nan_at_run_start")
                    elif np.isnan(Ms[s:e_]).any():
                        g.add("sg_nan_later_skipped")
                    if (Ms[s:e_] == -INF).all():
                        assert pk == s
                        g.add("sg_ninf_run")
                    continue
                if len(rr) > 1 and max(Ms[r[0]:r[1]].max() for r in rr[1:]) > Ms[pk]:
                    g.add("sg_later_run_higher")
                if len(rr) > 1 and max(r[1] - r[0] for r in rr[1:]) > e_ - s:
                    g.add("sg_later_run_longer")
                if (Ms[s:e_] == Ms[pk]).sum() > 1:
                    g.add("sg_equal_value_later")
                if c.params[0] is not None and e_ == hi and hi < n and mask[hi]:
                    g.add("sg_run_cut_by_bound_hi")
                if c.params[0] is not None and s == lo and lo > 0:
                    g.add("sg_run_starts_at_bound_lo" if not mask[lo - 1] else "sg_run_cut_by_bound_lo")
                if mask.all():
                    g.add("sg_all_true")
    return got


def required(n):
    """{fact: arithmetic predicate on n under which the streams must hold it}; the reason stands beside
    each predicate that is not simply True."""
    big = n >= 255                     # every constructed family fits: the longest needs 2 * 32 + 6 samples
    C = chunk(n)
    edges = C >= 3                     # n = 513, 1025: a residue 1 and a residue C - 1 that differ from 0
    req = {
        "plateau": {
            "pl_branch1": n >= 2,      # post_hi > center + 1 needs a second sample
            "pl_branch2": True,        # n = 1: w = 8 spreads the sample over a run of 8
            "pl_branch3": True, "pl_branch4": True,
            "pl_raise": n >= 7,        # zeros, cp 0, lookahead n + 2: a window of n - 3 >= 2 against none
            "pl_slice_wraps": n >= 7,
            "pl_n<w": n < 16,
            "pl_center_tie_d<64": n >= 2,
            "pl_center_tie_64<=d<256": n >= 255, "pl_center_tie_d>=256": n >= 257,   # tie_ends: d = n - 1
            "pl_center_tie_same_thread": n >= 257,                                   # tie+256, or tie_ends at 257
            "pl_center_last_skips_95": n >= 2,
            "pl_drop_tie": n >= 7,
            "pl_95_equal_last_in_window": n >= 9, "pl_95_equal_first_outside": n >= 9,   # p = 0, cp = 8
            "pl_60_equal_in_run": big, "pl_run_equals_min_run": big, "pl_short_run_before": big,
            "pl_only_short_run": big, "pl_two_long_runs": big, "pl_run_to_end": big,
        },
        "minn": {
            "mn_status0": True, "mn_status-2": True,
            # two_equal_runs: runs of 2 at [2, 4) and [6, 8), all of the first on the level and tied
            "mn_longest_tie": n >= 8, "mn_level_equal_in_gate": n >= 8, "mn_peak_tie_in_gate": n >= 8,
            "mn_bounds_cut_both_ends": big, "mn_bounds_remove_gate": big,
            "mn_longest_tie_in_one_chunk": C >= 3,     # pair_in_chunk: runs at 10 C and 10 C + 2
        },
        "gate": {
            "gt_max>0": True, "gt_max=0": True, "gt_max<0": True, "gt_seeded_by_argmax": True,
            "gt_seed_tie": n >= 2,
            "gt_quotient_equal": n >= 2, "gt_divide_differs_from_multiply": n >= 2,
            "gt_one_sixteenth_below": n >= 7, "gt_span_to_last": n >= 2,
        },
        "seg": {
            "sg_empty_status-1": True, "sg_all_true": True,
            "sg_later_run_higher": big, "sg_later_run_longer": big, "sg_equal_value_later": n >= 7,
            "sg_run_cut_by_bound_hi": big, "sg_run_starts_at_bound_lo": big, "sg_run_cut_by_bound_lo": big,
        },
        "nonfinite": {
            "pl_all_nan": True, "pl_all_ninf": True,
            "pl_ms_nan_from_inf": n >= 7,          # +inf and -inf at n // 2 and n // 2 + 1, one window of w >= 2
            "pl_nan_branch3": n >= 2, "pl_partial_nan_fallback": n >= 7,
            "mn_nan_is_peak": True, "mn_all_ninf_status-2": True, "mn_pinf_peak": n >= 2,
            "gt_all_nan_or_ninf_seed0": True, "gt_nan_unnormalised": n >= 2, "gt_nan_seeded": n >= 2,
            "sg_nan_at_run_start": True, "sg_nan_later_skipped": n >= 7, "sg_ninf_run": True,
        },
    }
    for op in ("pl", "mn"):
        for tag in ("start", "end"):
            for nm in ("0", "1", "C-1"):
                req["plateau" if op == "pl" else "minn"][f"{op}_run_{tag}%C={nm}"] = edges
    return req


def check(n):
    """Preconditions (grid, exact Ms, run() without a mutation equals the oracle) and every required fact
    present; returns {family group: facts found}."""
    _preconditions(n)
    got, req = facts(n), required(n)
    missing = sorted((k, f) for k, fs in req.items() for f, need in fs.items() if need and f not in got[k])
    assert not missing, (n, missing)
    return got
