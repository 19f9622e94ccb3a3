"""Exact streams for the CP-correlation helpers: ofs_cp_search (csrc/cp_search.hip, modes OFS_CPS_ROBUST and
OFS_CPS_PEAK) and ofs_cp_cfo (cp_cfo_kernel in csrc/ofdmsync.hip).

NumPy and the CPU oracle only.  A stream is [nb, T] complex with small integer components (|.| <= 7, so the
same samples are fed as complex128, complex64 and int16).  With P_w(d) = sum_br sum_{n<w} x[d+n] conj(x[d+n+N]),
a pair x[p] = a, x[p+N] = b in an otherwise zero stream adds a conj(b) to P_w(d) for every d in (p - w, p]:
a plateau of w bit-identical windows.  Every partial sum is an integer far below 2^53, so P(d), and in robust
mode sum_d P(d), are exact in any summation order and the expected P is compared bit for bit.  Expected
results always come from ofdm_oracle (cp_search, which is the loop of cp_cfo_robust / cp_cfo_peak, and
cp_cfo), never from the pattern a stream was built from; find_cp_start is checked to give the same index.

A Case is one launch: op "search" (mode 0 robust / 1 peak; one N, w, span; est per stream) or op "cfo"
(w is cp_len, est the CP starts).  cases() lists them, expected(j) holds the oracle's results of case j,
check() asserts the preconditions and that every fact required(cfg) asks for is present, and MUTANTS are
single wrong decisions applied to search(), the kernel's three-stage decision restated (strict > inside a
thread, then larger |P| / smaller d across the lanes of a wave, then across the four waves); each must change
the expected result of a stream of the family built for it (mutants_caught).

Why a tie does not depend on how a hypot rounds: the windows that share the largest integer |P|^2 of a range
are bit-identical, or axis-aligned (+-a + 0i, 0 +- ai) for which hypot is exact by IEEE 754; every other window
has an integer |P|^2 that is smaller by at least 1, and every |P|^2 is below 2^44, so its |P| is smaller by a
relative 2^-45 at least - 256 ulp, far beyond a 1-ulp difference between two hypot implementations.  No tie
rests on a 3-4-5 coincidence.  The non-finite family is kept out of this check; for it status and d are compared
exactly, cfo and P by NaN-ness and by value elsewhere.
"""
import functools
import math
from collections import Counter, namedtuple

import numpy as np

import ofdm_oracle as O

SW = 256                                   # threads per stream in cp_search.hip
WG = 256                                   # threads per stream of cp_cfo_kernel
FS = 1.0e6
T_MAIN = 800                               # holds d_hi = 650, the longest window pair (N + w = 128) and a margin
SPAN_MAIN, EST_MAIN = 300, 350             # d_lo = 50, d_hi = 650: 600 offsets, more than two strides
CONFIGS = ((8, 1, 1), (16, 3, 2), (8, 8, 3), (64, 64, 1), (16, 64, 2))     # (N, w, nb)
SPANS = (1, 20, 32, 128, 129, 300)         # 2 * span offsets when nothing clips: 2, 40, 64, 256, 258, 600
ROBUST, PEAK = 0, 1
NAN, INF = float("nan"), float("inf")
SENTINEL = 2 ** 63 - 1
ANGLE_TOL = 4.2e-12                        # rad: 1e-8 Hz at fs = 30.72 MHz, N = 2048 (test_cp_search_vs_reference_golden)

Case = namedtuple("Case", "op family mode N w nb T span names x est")


def cfo_tol(N, fs=FS):
    return ANGLE_TOL * fs / (2 * math.pi * N)


# ------------------------------------------------------------------------------------------
# stream builders
# ------------------------------------------------------------------------------------------
def _zeros(nb, T=T_MAIN):
    return np.zeros((nb, T), complex)


def _spot(x, N, w, s, a, b, br=0):
    """One pair: P_w(d) gains a conj(b) for d in [s, s + w)."""
    p = s + w - 1
    assert x[br, p] == 0 and x[br, p + N] == 0, (br, p)
    x[br, p], x[br, p + N] = a, b


def _cross(x, N, w, lo, k, a=3, b=2):
    """A plateau that holds the offsets lo + k and lo + k + 1."""
    if w == 1:
        _spot(x, N, w, lo + k, a, b)
        _spot(x, N, w, lo + k + 1, a, b)
    else:
        _spot(x, N, w, lo + k - (w - 1) // 2, a, b)


def _rand(nb, seed, T=T_MAIN, lo=-7):
    return np.random.default_rng(seed).integers(lo, 8, (nb, T, 2)).astype(float).view(complex)[..., 0]


def _rand_untied(nb, seed, N, w, S, es, T=T_MAIN):
    """_rand of the first seed in seed, seed + 1000, ... whose largest |P|^2 in every range [e - S, e + S) is
    held by bit-identical or axis-aligned windows only (the precondition check() asserts for every stream)."""
    U = T - (N + w)
    for k in range(400):
        x = _rand(nb, seed + 1000 * k, T)
        wr, wi = int_windows(x, N, w)
        m2 = wr * wr + wi * wi
        for e in es:
            lo, hi = max(0, e - S), min(U, e + S)
            if hi > lo:
                at = lo + np.flatnonzero(m2[lo:hi] == m2[lo:hi].max())
                if len({(int(wr[k_]), int(wi[k_])) for k_ in at}) > 1 and not np.all((wr[at] == 0) | (wi[at] == 0)):
                    break
        else:
            return x
    raise AssertionError((nb, seed, N, w, S))


PHASES = ((3, 2), (3j, 2), (-3, 2), (-3j, 2))          # a conj(b) = 6, 6i, -6, -6i


def fam_ties(N, w, nb):
    lo, g = EST_MAIN - SPAN_MAIN, w + 5
    out = []

    def add(name, fill, distract=True):
        x = _zeros(nb)
        fill(x)
        if distract:
            _spot(x, N, w, lo + 450, 2, 1, nb - 1)     # a lower plateau behind everything
        out.append((name, x, EST_MAIN))

    add("lane", lambda x: _cross(x, N, w, lo, 5))
    add("wave", lambda x: _cross(x, N, w, lo, 63))
    add("stride", lambda x: _cross(x, N, w, lo, 255))
    add("stride2", lambda x: _cross(x, N, w, lo, 511))

    def two(s1, s2):
        def fill(x):
            _spot(x, N, w, lo + s1, 3, 2)
            _spot(x, N, w, lo + s2, 3, 2, nb - 1)
        return fill

    add("same_thread", two(7, 7 + SW))
    add("two_lanes_or_waves", two(3, 3 + g))
    add("two_waves", two(10, 10 + 2 * g))
    add("second_pass_lane", two(40, 10 + SW))          # thread 10's second pass against thread 40's first
    add("second_pass_wave", two(200, 10 + SW))
    add("third_pass", two(100, 20 + 2 * SW))
    add("first_offset", two(0, 300), distract=False)
    add("last_offset", lambda x: _spot(x, N, w, lo + 2 * SPAN_MAIN - 1, 3, 2))
    return out


def fam_axis(N, w, nb):
    lo, g = EST_MAIN - SPAN_MAIN, w + 5
    out = []
    for j, (s1, s2) in enumerate(((10, 10 + g), (100, 10 + SW), (7, 7 + SW), (70, 330))):
        for k in range(4):
            x = _zeros(nb)
            _spot(x, N, w, lo + s1, *PHASES[k])
            _spot(x, N, w, lo + s2, *PHASES[(k + 1 + j % 3) % 4], nb - 1)    # another phase, never the same
            out.append((f"axis{j}_{k}", x, EST_MAIN))
    return out


def fam_branch(N, w, nb):
    lo = EST_MAIN - SPAN_MAIN
    out = []
    for name, second, (a3, b3) in (("cancel", (-3, 2), (2, 2)), ("quadrature", (3j, 2), (5, 2))):
        for s1, s2 in ((20, 150), (150, 20)):
            x = _zeros(nb)
            _spot(x, N, w, lo + s1, 3, 2, 0)
            _spot(x, N, w, lo + s1, *second, 1)
            _spot(x, N, w, lo + s2, a3, b3, nb - 1)
            out.append((f"{name}_{s1}", x, EST_MAIN))
    return out


def fam_halfopen(N, w, nb):
    lo, hi = EST_MAIN - SPAN_MAIN, EST_MAIN + SPAN_MAIN
    out = []
    for name, s in (("at_hi-1", hi - 1), ("at_hi", hi), ("at_hi-2", hi - 2)):
        x = _zeros(nb)
        _spot(x, N, w, s, 3, 2)
        _spot(x, N, w, lo + 30, 2, 1, nb - 1)
        out.append((name, x, EST_MAIN))
    return out


def fam_zsum(N, w, nb):
    lo = EST_MAIN - SPAN_MAIN
    out = [("zeros", _zeros(nb), EST_MAIN)]
    for name, k in (("real", 0), ("imag", 1)):
        x = _zeros(nb)
        _spot(x, N, w, lo + 20, *PHASES[k])
        _spot(x, N, w, lo + 300, *PHASES[k + 2], nb - 1)
        out.append((f"cancel_{name}", x, EST_MAIN))
    x = _zeros(nb)
    _spot(x, N, w, lo + 20, 3, 2)
    _spot(x, N, w, lo + 300, -3, 1, nb - 1)
    out.append(("no_cancel", x, EST_MAIN))
    return out


def ests(N, w, S, T=T_MAIN):
    U = T - (N + w)
    return (S, S - 1, 0, -1, 1 - S, U - S, U - S + 1, U, U + S - 1, U + S, T, T + 5, 400)


def fam_ranges(N, w, nb, S):
    out = []
    es = ests(N, w, S)
    pool = (("zero", _zeros(nb)), ("r0", _rand_untied(nb, 100 * N + w, N, w, S, es)),
            ("r1", _rand_untied(nb, 100 * N + w + 1, N, w, S, es)))
    for e in dict.fromkeys(ests(N, w, S)):               # S = 1 names some estimate twice
        for nm, x in pool:
            out.append((f"{nm}@{e}", x, e))
    return out


def fam_many(N, w, nb, S):
    """211 streams (a prime), every one its own samples and estimate, from before the stream to behind it."""
    es = np.linspace(-S - 3, T_MAIN + S + 3, 211).astype(int)
    return [(f"m{j}@{e}", _rand_untied(nb, 7000 + j, N, w, S, [int(e)]), int(e)) for j, e in enumerate(es)]


def fam_empty(N, w, nb):
    """span 0 (d_hi == d_lo), and through fam_empty_far / fam_empty_short d_hi < d_lo and T < N + w."""
    x = _rand(nb, 31)
    return [("span0@100", x, 100), ("span0@0", x, 0), ("span0@T", x, T_MAIN), ("span0@-3", x, -3)]


def fam_empty_far(N, w, nb):
    U = T_MAIN - (N + w)
    x = _rand(nb, 32)
    return [("beyond", x, U + 50), ("at_edge", x, U + 10), ("before", x, -10), ("far_before", x, -400)]


def fam_nonfinite(N, w, nb, S, est=EST_MAIN):
    """One non-finite sample (or a whole non-finite stream) around a range [est - S, est + S)."""
    lo, hi = est - S, est + S
    base = _rand(nb, 50 + w, lo=1)                       # no zero component: inf * sample is never NaN by 0 * inf
    zbg = _zeros(nb)
    _spot(zbg, N, w, lo + min(3, 2 * S - 1), 3, 2)
    out = []

    def put(name, pairs, src=base):
        x = src.copy()
        for br, i, v in pairs:
            x[br, i] = v
        out.append((name, x, est))

    put("nan_in_every_window", [(0, hi - 1, NAN)])       # with S = w // 2 the range is w wide: every window holds hi - 1
    put("nan_stream", [(br, slice(None), NAN) for br in range(nb)])
    put("nan_first_window", [(0, lo, NAN)])
    put("nan_last_window", [(nb - 1, hi - 1 + w - 1, NAN)])
    put("nan_b_side", [(0, est + N, NAN)])
    put("nan_imag_only", [(0, est, complex(2, NAN))])
    put("nan_zero_bg", [(0, est, NAN)], zbg)
    put("inf", [(0, est, INF)])
    put("ninf", [(nb - 1, est, -INF)])
    put("inf_imag", [(0, est, complex(3, INF))])
    put("inf_pair", [(0, est, INF), (nb - 1, est + 1, -INF)])
    put("inf_zero_bg", [(0, est, INF)], zbg)
    put("inf_b_side", [(0, lo + N, INF)])
    put("inf_then_nan", [(0, lo, INF), (0, hi - 1 + w - 1, NAN)])
    return out


CFO_LENS = (0, 1, 3, 64, WG - 1, WG, WG + 1, 2 * WG + 5)
T_CFO = 700


def fam_cfo(N, nb, cp):
    last = T_CFO - N - cp
    pool = [_rand(nb, 900 + N + cp + j, T_CFO) for j in range(2)]
    out = [(f"r{j}@{s}", pool[j], s) for j in range(2) for s in (0, last, last // 2, 1)]
    x = _zeros(nb, T_CFO)
    if cp:
        x[0, 5], x[0, 5 + N] = 3j, 2
    out.append(("pair@5", x, 5))
    out.append(("zero@0", _zeros(nb, T_CFO), 0))
    return out[:1] if (N, nb, cp) == (8, 1, 3) else out  # one launch of a single stream


# ------------------------------------------------------------------------------------------
# cases: one launch each
# ------------------------------------------------------------------------------------------
def _case(op, family, mode, N, w, nb, span, rows, T=T_MAIN):
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names), (family, names)
    x = np.array([r[1] for r in rows]).reshape(len(rows), nb, T)
    x.setflags(write=False)
    est = np.array([r[2] for r in rows], np.int64)
    est.setflags(write=False)
    return Case(op, family, mode, N, w, nb, T, span, tuple(names), x, est)


@functools.lru_cache(maxsize=None)
def cases():
    """Every launch; arrays are read-only (shared by every test)."""
    out = []
    for N, w, nb in CONFIGS:
        c = (N, w, nb)
        out.append(_case("search", "ties", PEAK, *c, SPAN_MAIN, fam_ties(*c)))
        out.append(_case("search", "axis", PEAK, *c, SPAN_MAIN, fam_axis(*c)))
        out.append(_case("search", "halfopen", PEAK, *c, SPAN_MAIN, fam_halfopen(*c)))
        if nb >= 2:
            out.append(_case("search", "branch", PEAK, *c, SPAN_MAIN, fam_branch(*c)))
        for mode in (ROBUST, PEAK):
            out.append(_case("search", "zsum", mode, *c, SPAN_MAIN, fam_zsum(*c)))
            for S in SPANS:
                out.append(_case("search", "ranges", mode, *c, S, fam_ranges(*c, S)))
            out.append(_case("search", "empty", mode, *c, 0, fam_empty(*c)))
            out.append(_case("search", "empty", mode, *c, 10, fam_empty_far(*c)))
            Ts = N + w - 1                                  # T < N + w: no window fits
            out.append(_case("search", "empty", mode, *c, 5, [("short@0", _rand(nb, 33, Ts), 0),
                                                              ("short@2", _rand(nb, 34, Ts), 2)], T=Ts))
            Tf = N + w + 1                                  # the shortest stream with a range: [0, 1)
            out.append(_case("search", "ranges", mode, *c, 5, [("fit@0", _rand(nb, 35, Tf), 0),
                                                               ("fit@3", _rand(nb, 36, Tf), 3)], T=Tf))
            if w >= 2:
                out.append(_case("search", "nonfinite", mode, *c, w // 2, fam_nonfinite(*c, w // 2)))
            out.append(_case("search", "nonfinite", mode, *c, SPAN_MAIN, fam_nonfinite(*c, SPAN_MAIN)))
    for mode in (ROBUST, PEAK):
        out.append(_case("search", "ranges", mode, 16, 3, 2, 20, fam_many(16, 3, 2, 20)))
    for N, nb in ((8, 1), (64, 2), (16, 3)):
        for cp in CFO_LENS:
            out.append(_case("cfo", "cfo", None, N, cp, nb, None, fam_cfo(N, nb, cp), T=T_CFO))
    return tuple(out)


def is_finite(case):
    return case.family != "nonfinite"


def oracle(case, b):
    """(status, d, P, cfo) of stream b from ofdm_oracle."""
    x, e = case.x[b], int(case.est[b])
    with np.errstate(all="ignore"):
        if case.op == "cfo":
            cfo, P = O.cp_cfo(x, e, case.N, case.w, FS)
            return 0, e, P, cfo
        return O.cp_search(x, e, case.N, case.w, case.span, case.mode, FS)


@functools.lru_cache(maxsize=None)
def expected(j):
    c = cases()[j]
    return tuple(oracle(c, b) for b in range(len(c.names)))


# ------------------------------------------------------------------------------------------
# comparison: the one rule of the GPU test
# ------------------------------------------------------------------------------------------
def _bits(v):
    return np.float64(v).view(np.int64)


def cfo_same(gc, ec, N, fs=FS):
    """NaN where the oracle's is, -0.0 / +0.0 where the oracle's is, else within cfo_tol."""
    gc, ec = float(gc), float(ec)
    if math.isnan(ec) or math.isnan(gc):
        return math.isnan(ec) and math.isnan(gc)
    if ec == 0.0:
        return gc == 0.0 and math.copysign(1.0, gc) == math.copysign(1.0, ec)
    return abs(gc - ec) <= cfo_tol(N, fs)


def same(got, exp, N, exact=True, fs=FS):
    """status and d equal; P bit for bit (exact) or equal with NaNs equal by component; cfo as cfo_same."""
    (gs, gd, gP, gc), (es, ed, eP, ec) = got, exp
    if int(gs) != es or int(gd) != ed:
        return False
    gP, eP = complex(gP), complex(eP)
    for g, e in ((gP.real, eP.real), (gP.imag, eP.imag)):
        if math.isnan(e) or math.isnan(g):
            if not (math.isnan(e) and math.isnan(g)):
                return False
        elif (_bits(g) != _bits(e)) if exact else (g != e):
            return False
    return cfo_same(gc, ec, N, fs)


# ------------------------------------------------------------------------------------------
# the kernel's decision restated, and its mutants
# ------------------------------------------------------------------------------------------
def _windows(x, N, w, lo, hi):
    """(pr, pi)[br, d - lo] for d in [lo, hi) in the kernel's real arithmetic; x is zero outside [0, T)."""
    nb, T = x.shape
    nd = hi - lo
    if w == 0 or nd <= 0:
        return np.zeros((nb, max(nd, 0))), np.zeros((nb, max(nd, 0)))
    padl, padr = max(0, -lo), max(0, hi + w + N - T)
    xp = np.concatenate([np.zeros((nb, padl)), x, np.zeros((nb, padr))], axis=1)
    u = xp[:, lo + padl:hi + padl + w - 1]
    v = xp[:, lo + padl + N:hi + padl + w - 1 + N]
    tr = u.real * v.real + u.imag * v.imag                  # u * conj(v)
    ti = u.imag * v.real - u.real * v.imag
    sw = np.lib.stride_tricks.sliding_window_view
    return sw(tr, w, axis=1).sum(axis=2), sw(ti, w, axis=1).sum(axis=2)


def search(x, est, N, w, span, mode, fs=FS, mut=None):
    """cp_search_kernel restated: (status, d, P, cfo)."""
    with np.errstate(all="ignore"):
        T = x.shape[1]
        d_lo = est - span if mut == "lo_unclipped" else max(0, est - span)
        d_hi = min(T - (N + (2 * w if mut == "hi_cp_len" else w)), est + span)
        if d_hi <= d_lo and mut != "empty_unreported":
            return 1, est, complex(NAN, NAN), NAN
        end = d_hi + 1 if mut == "hi_inclusive" else d_hi
        pr, pi = _windows(x, N, w + {"win_short": -1, "win_long": 1}.get(mut, 0), d_lo, end)
        if mut == "conj_wrong":
            pi = -pi
        if mut == "abs_per_branch":
            mag = np.hypot(pr, pi).sum(axis=0)
        pr, pi = pr.sum(axis=0), pi.sum(axis=0)
        if mut != "abs_per_branch":
            mag = np.hypot(pr, pi)
        nd = max(0, end - d_lo)
        if mode == ROBUST:
            wr = [sum(float(v) for t in range(64 * k, 64 * k + 64) for v in pr[t::SW]) for k in range(SW // 64)]
            wi = [sum(float(v) for t in range(64 * k, 64 * k + 64) for v in pi[t::SW]) for k in range(SW // 64)]
            br, bi, bd = 0.0 + sum(wr), 0.0 + sum(wi), est
        else:
            cand = []                                        # per thread: (key, d, pr, pi)
            for t in range(SW):
                key, bd, br, bi = -1.0, SENTINEL, 0.0, 0.0
                for k in range(t, nd, SW):
                    if (mag[k] >= key) if mut == "ge" else (mag[k] > key):
                        key, bd, br, bi = float(mag[k]), d_lo + k, float(pr[k]), float(pi[k])
                cand.append((key, bd, br, bi))

            def reduce(items, larger_d):
                best = items[0]
                for it in items[1:]:
                    if it[0] > best[0] or (it[0] == best[0] and ((it[1] > best[1]) if larger_d else (it[1] < best[1]))):
                        best = it
                return best

            waves = [reduce(cand[64 * k:64 * k + 64], mut == "larger_d_lanes") for k in range(SW // 64)]
            key, bd, br, bi = reduce(waves, mut == "larger_d_waves")
            if bd == SENTINEL and mut != "nan_sentinel":     # no comparable window: core.py:289-291 keeps d_lo, 0j
                bd = d_lo
        return 0, bd, complex(br, bi), -math.atan2(bi, br) * fs / (2.0 * math.pi * N)


def run(case, b, mut=None):
    return search(case.x[b], int(case.est[b]), case.N, case.w, case.span, case.mode, FS, mut)


# mutant -> (mode, family) built for it
MUTANTS = {
    "ge": (PEAK, "ties"),
    "larger_d_lanes": (PEAK, "ties"),
    "larger_d_waves": (PEAK, "ties"),
    "hi_inclusive": (PEAK, "halfopen"),
    "lo_unclipped": (PEAK, "ranges"),
    "hi_cp_len": (ROBUST, "ranges"),
    "win_short": (PEAK, "ties"),
    "win_long": (PEAK, "ties"),
    "conj_wrong": (PEAK, "axis"),
    "abs_per_branch": (PEAK, "branch"),
    "nan_sentinel": (PEAK, "nonfinite"),
    "empty_unreported": (PEAK, "empty"),
}
# further (mutant, mode, family) that must be caught as well
TARGETS = (("ge", PEAK, "axis"), ("larger_d_waves", PEAK, "axis"), ("hi_inclusive", ROBUST, "ranges"),
           ("lo_unclipped", ROBUST, "ranges"), ("hi_cp_len", PEAK, "ranges"), ("win_short", ROBUST, "ranges"),
           ("win_long", ROBUST, "ranges"), ("conj_wrong", ROBUST, "ranges"), ("empty_unreported", ROBUST, "empty"))


def mutants_caught():
    """{(mutant, mode, family): [(N, w, nb, span, stream)] whose expected result the mutant changes}."""
    out = {}
    cs = cases()
    for mut, mode, fam in [(m, *v) for m, v in MUTANTS.items()] + list(TARGETS):
        hit = []
        for j, c in enumerate(cs):
            if c.op != "search" or c.family != fam or c.mode != mode or len(c.names) > 100:
                continue
            exp = expected(j)
            hit += [(c.N, c.w, c.nb, c.span, c.names[b]) for b in range(len(c.names))
                    if not same(run(c, b, mut), exp[b], c.N, exact=is_finite(c))]
        out[(mut, mode, fam)] = hit
    return out


# ------------------------------------------------------------------------------------------
# check(): preconditions and coverage
# ------------------------------------------------------------------------------------------
def int_windows(x, N, w):
    """Exact integer (re, im) of P_w(d) for d in [0, T - N - w]; x holds integers."""
    xr, xi = np.rint(x.real).astype(np.int64), np.rint(x.imag).astype(np.int64)
    n = x.shape[1] - N
    tr = (xr[:, :n] * xr[:, N:] + xi[:, :n] * xi[:, N:]).sum(axis=0)
    ti = (xi[:, :n] * xr[:, N:] - xr[:, :n] * xi[:, N:]).sum(axis=0)
    cr, ci = np.concatenate([[0], np.cumsum(tr)]), np.concatenate([[0], np.cumsum(ti)])
    return cr[w:] - cr[:n - w + 1], ci[w:] - ci[:n - w + 1]


def _range(c, b):
    e = int(c.est[b])
    return max(0, e - c.span), min(c.T - (c.N + c.w), e + c.span)


class _Facts(Counter):
    """fact -> number of streams that hold it."""
    def next_stream(self):
        self._seen = set()

    def add(self, fact):
        if fact not in self._seen:
            self._seen.add(fact)
            self[fact] += 1


def check_and_facts():
    """Asserts the preconditions of every case and returns {(N, w, nb) or "cfo": {fact: streams that hold it}}."""
    got = {}
    for j, c in enumerate(cases()):
        exp = expected(j)
        g = got.setdefault("cfo" if c.op == "cfo" else (c.N, c.w, c.nb), _Facts())
        assert c.x.shape == (len(c.names), c.nb, c.T) and not c.x.flags.writeable
        fin = np.isfinite(c.x.real) & np.isfinite(c.x.imag)
        v = np.stack([c.x.real[fin], c.x.imag[fin]])
        assert np.all(v == np.rint(v)) and np.all(np.abs(v) <= 7), c.family          # int16 and float32 hold them
        assert fin.all() or not is_finite(c), c.family
        if c.op == "cfo":
            for b, name in enumerate(c.names):
                g.next_stream()
                st, d, P, cfo = exp[b]
                assert 0 <= d and d + c.N + c.w <= c.T
                wr, wi = int_windows(c.x[b], c.N, c.w) if c.w else ([0] * c.T, [0] * c.T)
                assert _bits(P.real) == _bits(float(wr[d])) and _bits(P.imag) == _bits(float(wi[d])), name
                g.add(f"cfo_len{c.w}" if c.w < 2 else "cfo_len<WG" if c.w < WG else "cfo_len=WG" if c.w == WG else
                      "cfo_len>WG")
                g.add(f"cfo_nb{c.nb}")
                g.add("cfo_start0" if d == 0 else "cfo_start_last" if d == c.T - c.N - c.w else "cfo_start_mid")
                if P == 0 and math.copysign(1.0, cfo) < 0:
                    g.add("cfo_zero_is_-0.0")
                g.add(f"cfo_B{min(len(c.names), 2)}")
            continue
        for b, name in enumerate(c.names):
            tag = (c.family, c.mode, c.N, c.w, c.span, name)
            g.next_stream()
            st, d, P, cfo = exp[b]
            e = int(c.est[b])
            lo, hi = _range(c, b)
            assert same(run(c, b), exp[b], c.N, exact=is_finite(c)), tag           # the restated search is the oracle
            if c.mode == PEAK and st == 0:
                with np.errstate(all="ignore"):
                    assert O.find_cp_start(c.x[b], e, c.N, c.w, c.span) == d, tag
                    assert O.cp_cfo_peak(c.x[b], e, c.N, c.w, FS, span=c.span) == (cfo, d) or math.isnan(cfo), tag
            if st == 1:
                assert hi <= lo and d == e and math.isnan(cfo) and math.isnan(P.real) and math.isnan(P.imag), tag
                g.add("empty_eq" if hi == lo else "empty_T<N+w" if c.T < c.N + c.w else "empty_lt")
                continue
            n = hi - lo
            g.add("range_1" if n == 1 else "range_<64" if n < 64 else "range_64" if n == 64 else
                  f"range_{n}" if n in (255, 256, 257) else "range_65..254" if n < 255 else
                  "range_258..512" if n <= 512 else "range_>512")
            if e - c.span < 0:
                g.add("clip_lo")
            if e + c.span > c.T - (c.N + c.w):
                g.add("clip_hi")
            if e < 0:
                g.add("est<0")
            if e >= c.T:
                g.add("est>=T")
            if not is_finite(c):
                _nonfinite_facts(g, c, b, exp[b], lo, hi)
                continue
            wr, wi = int_windows(c.x[b], c.N, c.w)
            wr, wi = [int(v_) for v_ in wr[lo:hi]], [int(v_) for v_ in wi[lo:hi]]
            assert not (math.copysign(1.0, P.real) < 0 and P.real == 0) and not (math.copysign(1.0, P.imag) < 0 and P.imag == 0)
            if c.mode == ROBUST:
                assert (P.real, P.imag) == (float(sum(wr)), float(sum(wi))) and abs(sum(wr)) + abs(sum(wi)) < 2 ** 50, tag
                if P == 0 and any(wr) and math.copysign(1.0, cfo) < 0:
                    g.add("robust_sum_zero")
                continue
            m2 = [r * r + i * i for r, i in zip(wr, wi)]
            top = max(m2)
            assert top < 2 ** 44, tag
            at = [k for k, v_ in enumerate(m2) if v_ == top]
            tied = {(wr[k], wi[k]) for k in at}
            assert len(tied) == 1 or all(r == 0 or i == 0 for r, i in tied), tag     # bit-identical or axis-aligned
            assert d == lo + at[0] and (P.real, P.imag) == (wr[at[0]], wi[at[0]]), tag
            if top == 0:
                assert d == lo and math.copysign(1.0, cfo) < 0 and cfo == 0
                g.add("all_zero")
                continue
            if len(tied) > 1:
                g.add("tie_axis_phase")
            s = set(at)
            for k in at:
                if k + 1 in s and k // 64 == (k + 1) // 64:
                    g.add("tie_lane")
                if k + SW in s:
                    g.add("tie_same_thread")
                if k < SW and any(SW <= k2 < 2 * SW and k2 - SW < k for k2 in at):
                    g.add("tie_second_pass_vs_higher_thread")
                if any(k2 // 64 != k // 64 and k2 // SW == k // SW for k2 in at):
                    g.add("tie_two_waves")
            for k, nm in ((63, "tie_wave"), (255, "tie_stride"), (511, "tie_stride2")):
                if k in s and k + 1 in s:
                    g.add(nm)
            if at[0] == 0:
                g.add("max_at_d_lo")
            if at[0] == n - 1:
                g.add("max_at_hi-1")
            full = int_windows(c.x[b], c.N, c.w)
            if hi < len(full[0]) and int(full[0][hi]) ** 2 + int(full[1][hi]) ** 2 > top:
                g.add("max_at_hi_excluded")
            if c.nb > 1 and c.family == "branch":
                per = [int_windows(c.x[b][r:r + 1], c.N, c.w) for r in range(c.nb)]
                if sum(math.hypot(int(p[0][d]), int(p[1][d])) for p in per) < max(
                        sum(math.hypot(int(p[0][k]), int(p[1][k])) for p in per) for k in range(lo, hi)):
                    g.add("branches_cancel")
    return got


def _nonfinite_facts(g, c, b, e, lo, hi):
    st, d, P, cfo = e
    x = c.x[b]
    with np.errstate(all="ignore"):
        pr, pi = _windows(x, c.N, c.w, lo, hi)
        mag = np.hypot(pr.sum(axis=0), pi.sum(axis=0))
    if c.mode == ROBUST:
        if math.isnan(cfo):
            g.add("nf_robust_nan")
        return
    if np.isnan(mag).all():
        assert d == lo and P == 0 and cfo == 0 and math.copysign(1.0, cfo) < 0, c.names[b]
        g.add("nf_all_nan_stream" if np.isnan(x).all() else "nf_all_nan_one_sample" if np.isnan(x).sum() == 1
              else "nf_all_nan")
        if c.span == c.w // 2:
            g.add("nf_all_nan_default_span")
    elif np.isnan(mag).any():
        g.add("nf_part_nan")
        if np.isnan(mag[0]):
            g.add("nf_part_nan_first_window")
        if np.isnan(mag[:d - lo]).any():
            g.add("nf_nan_before_answer")
    if np.isinf(x).any():
        g.add("nf_inf")
        if np.isinf(mag).any():
            assert np.isinf(abs(P)) and d == lo + int(np.flatnonzero(np.isinf(mag))[0]), c.names[b]
            g.add("nf_inf_wins")
            if np.isinf(mag).sum() > 1:
                g.add("nf_inf_tie")


TIE_FACTS = ("tie_lane", "tie_wave", "tie_stride", "tie_stride2", "tie_same_thread", "tie_two_waves",
             "tie_second_pass_vs_higher_thread", "tie_axis_phase", "all_zero", "max_at_d_lo", "max_at_hi-1",
             "max_at_hi_excluded", "robust_sum_zero")
RANGE_FACTS = ("range_1", "range_<64", "range_64", "range_255", "range_256", "range_257", "range_258..512",
               "range_>512", "clip_lo", "clip_hi", "est<0", "est>=T", "empty_eq", "empty_lt", "empty_T<N+w")
NF_FACTS = ("nf_all_nan_stream", "nf_part_nan", "nf_part_nan_first_window",
            "nf_nan_before_answer", "nf_inf", "nf_inf_wins", "nf_inf_tie", "nf_robust_nan")
CFO_FACTS = ("cfo_len0", "cfo_len1", "cfo_len<WG", "cfo_len=WG", "cfo_len>WG", "cfo_nb1", "cfo_nb2", "cfo_nb3",
             "cfo_start0", "cfo_start_last", "cfo_start_mid", "cfo_zero_is_-0.0", "cfo_B1", "cfo_B2")


def required(cfg):
    """The facts a configuration must hold: all of them, except what its shape cannot hold (reason beside)."""
    if cfg == "cfo":
        return set(CFO_FACTS)
    N, w, nb = cfg
    req = set(TIE_FACTS + RANGE_FACTS + NF_FACTS)
    if nb >= 2:
        req.add("branches_cancel")                         # needs a second branch
    if w >= 2:
        req |= {"nf_all_nan_default_span", "nf_all_nan_one_sample"}   # span = w // 2 is 0 for w = 1: an empty range
    return req


def check():
    got = check_and_facts()
    missing = sorted((str(k), f) for k in got for f in required(k) if f not in got[k])
    assert not missing, missing
    return got
