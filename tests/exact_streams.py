"""Exact-arithmetic [A][A] streams (tests only; NumPy and the CPU oracle, no GPU).

Every sample is s[n] * u[n mod L] with u[k] in {1, j, -1, -j} and s[n] in {+1, -1, 0}.  Every
lagged product is then e[n] = s[n] s[n-L], so P[n] = v[n], the sliding sum of e (times j^b or (-1)^b
in the block-rotated streams), and R[n] = the number of non-zero samples in the window:
small integers.  fp32 and fp64 agree exactly on them in any summation order, and M = (v / r)^2 takes
few values, none of them near the threshold (check() asserts a margin of 1e-4, 100 x the tie
tolerance of oracle/parity.py).  Every [A][A] path must therefore give the oracle's events exactly.

A greedy builder (build()) follows a wanted above / below pattern sample by sample: with all samples
non-zero, v moves by +-1 per sample while the window fills (n < 2L) and by 0 or +-2 after (it can
hold, go down where e[n-L] = +1 and up where e[n-L] = -1).  Not every wanted flag can be met, so
scenarios are searched over their position until the ORACLE's events on the stream as built have the
wanted property, and the expected events always come from the oracle, never from the pattern.
Streams whose support is the first h phases of every period (zero elsewhere) behave like a window of
h samples and reach the threshold h-times sooner after n = L; they serve the shapes where T - L is
short.  A zero sample in the head (n < L) holds v for one step while the window fills, which
changes the parity of v against n.

streams(L, T, hyst, n_ant) is the set every test uses; check() asserts the preconditions and the
coverage of the gate machine's edges on the oracle's output.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import ofdm_oracle as O

THR = 0.15
FS = 15.36e6
MARGIN = 1e-4                      # min |M - thr| that check() asserts
BUILD_MARGIN = 1.5e-4              # what the builder keeps clear of
HYSTS = (0, 1, 2, 16, 127, 128, 129, 255, 256, 257, 511, 512, 513)
ROWS = (128, 512)                  # row lengths whose first / last lane must see a close
MAX_EVENTS = 4


# (L, T, n_ant) of every path of tests/test_gpu_aa_exact_events.py; tests/test_exact_streams_host.py
# runs check() on each with every hysteresis of hysts(T)
SHAPES = {
    "fast": [(128, 1024, 1), (256, 1024, 1), (512, 1024, 1)],                 # register-staged kernel, full stream
    "short": [(128, 640, 1), (256, 640, 1), (512, 640, 1), (128, 1022, 1), (256, 1022, 1), (512, 1022, 1)],
    "two": [(128, 1024, 2), (256, 1024, 2), (512, 1024, 2), (128, 768, 2), (256, 768, 2), (512, 768, 2)],
    # streaming kernels: every plan value 1121 / 1122 / 1124 / 1128, every T, one and two antennas
    "stream": [(128, 1023, 1), (128, 5315, 2), (256, 1025, 2), (512, 2047, 1), (1024, 1025, 1), (1024, 4096, 2)],
    "general": [(192, 1024, 1), (192, 2690, 1), (192, 3202, 1)],             # fused; tiled in fp32 / fp64
    "chunk": [(128, 1024, 1), (512, 2047, 1), (128, 420, 1)],
}


def all_shapes():
    return sorted({s for v in SHAPES.values() for s in v})


def hysts(T):
    """The hysteresis list of a stream length: HYSTS and one value above T (no gate closes before T)."""
    return HYSTS + (T + 7,)


class _Lcg:
    """Fixed pseudo-random integers (no dependence on a NumPy generator's stream)."""

    def __init__(self, seed):
        self.x = (seed * 2654435761 + 12345) & 0xFFFFFFFF

    def below(self, n):
        self.x = (1664525 * self.x + 1013904223) & 0xFFFFFFFF
        return (self.x >> 12) % max(int(n), 1)


def unit(L, seed):
    """u[0..L): entries of {1, j, -1, -j}.  (+-1 +- j would keep P and R integers too, but the
    reference's |x|^2 = abs(x)^2 is 2.0000000000000004 there, and R must be exact in every form.)"""
    g = _Lcg(seed)
    base = np.array([1, 1j, -1, -1j], np.complex128)
    return base[[g.below(4) for _ in range(L)]]


def build(L, T, want, thr=THR, h=None, active=None, jit=0, zero_at=()):
    """s[0..T) in {+1, -1, 0} following want[n] (0: below the threshold, w >= 1: above, as close
    to the threshold as it goes for w = 1 and 2 (w - 1) higher in v for w > 1) over the samples
    of ``active`` ([lo, hi) pairs; default: all) and holding v and r elsewhere where it can.
    ``h``: support, the phases n mod L < h are non-zero.  While the window fills and nothing is
    wanted yet, v follows a ramp to just under the threshold with an irregular walk seeded by ``jit``
    under it: that spreads the e = -1 phases (where v can step up later) over the whole period, and a
    regular +-+- hover would leave every later step down on an even phase and every step up on an
    odd one.  A crossing is only made where the crossing back can be made at the sample the pattern
    wants it (the sign of e one period before that sample; while the window fills, the parity of the
    distance).  ``zero_at``: head samples (< L) that are zero: v holds at zero_at + L, which changes
    the parity of v against n for the rest of the fill (r is one less before that sample)."""
    h = L if h is None else min(h, L)
    s = [0] * T
    for n in range(min(L, T)):
        s[n] = 1 if n < h and n not in zero_at else 0
    e = [0] * T
    act = np.ones(T, bool)
    if active is not None:
        act[:] = False
        for lo, hi in active:
            act[max(lo, 0):max(hi, 0)] = True
    act[:min(2 * L, T)] = True
    act = act.tolist()
    wa = np.asarray(want) > 0
    want = np.asarray(want).tolist()
    chg = np.flatnonzero(wa[1:] != wa[:-1]) + 1                        # where the wanted flag changes
    nxt = np.full(T, T, int)
    if len(chg):
        k = np.searchsorted(chg, np.arange(T), side="right")
        nxt = np.where(k < len(chg), chg[np.minimum(k, len(chg) - 1)], T)
    nxt = nxt.tolist()
    need = np.zeros(T, int)                                            # the sign of e that lets the pattern cross
    for c in chg:                                                      # one period later
        if c - L >= L:
            need[c - L] = -1 if wa[c] else 1
    need = need.tolist()
    sq = math.sqrt(thr)
    v, rc = 0, sum(1 for q in s[:L] if q)
    rnd = _Lcg(7919 * jit + L)
    soon = np.convolve(wa, np.ones(8, int))[7:]                        # an above sample within 7
    first = np.flatnonzero(wa)
    ramp_end = min(2 * L, (int(first[0]) if len(first) else T) - 8)
    sup_before = lambda n: (n // L) * h + min(n % L, h)                # support samples below n
    ramp_len = max(sup_before(ramp_end) - sup_before(L), 1)
    above = False
    for n in range(L, T):
        sp, ep = s[n - L], e[n - L]
        if not act[n] and sp != 0 and ep != 0 and n % L < h:
            s[n], e[n] = ep * sp, ep                          # hold: e[n] = e[n-L], v and r stay
            continue
        hold = False
        if n % L >= h:
            opts = (0,)
        elif not act[n] and sp == 0:
            opts = (0,)
            hold = True
        else:
            opts = (1, -1)
        best = None
        drift = rnd.below(5) if n < 2 * L else 0
        w = want[n]
        for o in opts:
            en = o * sp
            v2, r2 = v + en - ep, rc + (1 if o else 0) - (1 if sp else 0)
            m = min(v2 * v2 / (r2 * r2), 1.0) if r2 > 0 else 0.0
            b = sq * r2
            tgt = b - 0.5 if w == 0 else b + 0.5 + 2 * (w - 1)
            if w == 0 and n < 2 * L and not soon[n]:
                if n < ramp_end:
                    tgt *= min((sup_before(n + 1) - sup_before(L)) / ramp_len, 1.0)
                tgt -= drift
            ab2 = m >= thr
            blocked = False
            if ab2 != above and ab2 == (w > 0) and not hold and nxt[n] < T:
                back = nxt[n]                                 # where the pattern crosses back
                if back < 2 * L:
                    blocked = (back - n) % 2 == 0 and not any(n < z + L <= back for z in zero_at)
                elif back - L <= n:
                    eb = en if back - L == n else e[back - L]
                    blocked = eb != (1 if ab2 else -1) and s[back - L] != 0
            score = (abs(m - thr) < BUILD_MARGIN, blocked, ab2 != (w > 0), need[n] != 0 and en != need[n], abs(v2 - tgt))
            if best is None or score < best[0]:
                best = (score, o, en, v2, r2, ab2)
        _, s[n], e[n], v, rc, above = best
    return np.array(s, np.int8)


def samples(s, u, rot=0):
    """x[n] = s[n] u[n mod L] (rot = 1: block b times j^b, rot = 2: times (-1)^b) as int16 I/Q [T, 2]."""
    L, T = len(u), len(s)
    n = np.arange(T)
    x = s.astype(np.complex128) * u[n % L]
    if rot:
        x = x * (1j ** rot) ** (n // L)
    iq = np.stack([np.rint(x.real), np.rint(x.imag)], -1).astype(np.int16)
    assert np.array_equal(iq[:, 0] + 1j * iq[:, 1], x)
    return iq


def cplx(iq, dtype=np.complex128):
    """int16 I/Q [.., 2] -> complex (zeros are +0.0 in both parts)."""
    out = np.zeros(iq.shape[:-1], dtype)
    out.real = iq[..., 0]
    out.imag = iq[..., 1]
    return out


def _gates(iq, L, hyst):
    """(P, M, gates [k, 4] = (0, start, end, 0)) by the closed form of the gate machine: a gate opens
    at an above sample whose distance to the previous one exceeds Hp (or that has none), and closes
    Hp after its last above sample, or at T.  For the scenario search only: what a test expects
    always comes from the oracle's literal loop."""
    P, R, M, valid = O.aa_metric(cplx(iq), L)
    T, Hp = len(M), max(hyst, 1)
    idx = np.flatnonzero(M[L:] >= THR) + L
    if len(idx) == 0:
        return P, M, np.zeros((0, 4), np.int64)
    brk = np.flatnonzero(np.diff(idx) - 1 >= Hp)
    starts = idx[np.concatenate(([0], brk + 1))]
    last = idx[np.concatenate((brk, [len(idx) - 1]))]
    ends = np.minimum(last + Hp, T)
    z = np.zeros_like(starts)
    return P, M, np.stack([z, starts, ends, z], 1)


def amin(L, h):
    """First sample that can be above the threshold with support h (v = n - L + 1 reaches sqrt(thr) h)."""
    return L + math.ceil(math.sqrt(THR) * min(h, L)) - 1


def _supports(L):
    """Supports tried in turn: the whole period first, then the first 256 / 128 / 32 phases."""
    return sorted({h for h in (L, 256, 128, 32) if h <= L}, reverse=True)


def reachable(L, T, p):
    """Whether some support can place an above sample at p: behind that support's first possible
    above sample and on one of its phases."""
    return 0 <= p < T and any(p >= amin(L, h) + 1 and p % L < h for h in _supports(L))


def gap_fits(L, T, g):
    """Whether some support can hold above samples at a and a + g + 1 for some a."""
    return any(any(a % L < h and (a + g + 1) % L < h for a in range(amin(L, h) + 3, T - g - 4))
               for h in _supports(L))


def _span(L, T, lo, hi):
    """The samples the builder works on for a scenario on [lo, hi] (it holds elsewhere): from one
    period before, where the crossings are prepared."""
    return [(lo - L - 64, hi + 64)]


def _search(L, T, u, make, ok, positions, jits=(0, 1, 2), budget=600, hs=None):
    """The first support h, position p of ``positions``, head zeros and warm-up walk for which the
    stream built from make(p) satisfies ok (a property of the oracle's output on it); None if there
    is none.  make(p) returns (want, active, hold): ``hold`` is a sample while the window fills at
    which a one-step hold of v would mend the parity (or None)."""
    for h in (hs or _supports(L)):
        for p in positions:
            if p < amin(L, h) + 1 or p >= T:
                continue
            want, span, hold = make(p)
            zeros = [()]
            if hold is not None and L <= hold < 2 * L and hold - L < h:
                z = hold - L
                zeros += [(z,), (z, min(L, h) - 1), (z, min(L, h) - 1, min(L, h) - 2)]
            for jit in jits:
                for z in zeros:
                    budget -= 1
                    if budget < 0:
                        return None
                    iq = samples(build(L, T, want, h=h, active=span, jit=jit, zero_at=z), u)
                    if ok(iq, p):
                        return iq
    return None


def _from(lo, hi, seed, count=40):
    """Up to ``count`` distinct positions of [lo, hi]: a seeded start, then odd strides (both
    parities of the position), wrapping."""
    if hi < lo:
        return []
    n = hi - lo + 1
    start = _Lcg(seed).below(n)
    stride = max(n // count, 1) | 1
    out = []
    for i in range(min(count, n)):
        p = lo + (start + i * stride) % n
        if p not in out:
            out.append(p)
    return out


def gap_stream(L, T, g, u, seed):
    """Above at a, below on a+1 .. a+g, above at a+g+1, for some a."""
    def make(a, peaked=False):
        w = np.zeros(T, np.int8)
        w[max(a - 2, L):a + 1] = 1
        if peaked and a - 4 >= L:                             # up to a higher level and back: e[a-1] = -1
            w[a - 4:a + 1] = [1, 1, 2, 1, 1]
        w[a + g + 1:a + g + 4] = 1
        return w, _span(L, T, a, a + g), a + 1 + g // 2

    def ok(iq, a):
        M = O.aa_metric(cplx(iq), L)[2]
        idx = np.flatnonzero(M >= THR)
        return bool(np.any(np.diff(idx) - 1 == g)) if g > 0 else bool(np.any(np.diff(idx) == 1))

    out = None
    for h in _supports(L):                                    # positions behind the first possible above sample
        for mk in (make, lambda a: make(a, True)):
            if out is None:
                out = _search(L, T, u, mk, ok, _from(amin(L, h) + 3, T - g - 2, seed, 80), hs=(h,))
    return out


def pulse_stream(L, T, positions, u, hyst, pred, r=2, jits=(0, 1, 2)):
    """Above on p-r+1 .. p and below elsewhere, as far as it goes; pred(ev_int, P, M) decides."""
    def make(q):
        w = np.zeros(T, np.int8)
        w[max(q - r + 1, L):q + 1] = 1
        return w, _span(L, T, q, q), q - 24

    def ok(iq, q):
        P, M, ei = _gates(iq, L, hyst)
        return pred(ei, P, M)

    return _search(L, T, u, make, ok, positions, jits)


def pattern_stream(L, T, start, pattern, u, h=None):
    """want = pattern from ``start`` on (levels), below elsewhere."""
    w = np.zeros(T, np.int8)
    pat = np.asarray(pattern, np.int8)[:max(T - start, 0)]
    w[start:start + len(pat)] = pat
    return samples(build(L, T, w, h=h, active=_span(L, T, start, start + len(pat))), u)


def close_targets(L, T, hyst):
    """Per (RL, residue = RL - 1 or 0): the samples c < T of that residue at which a gate can close
    (its last above sample c - Hp lies behind the first that can be above), from a seeded start;
    residues without any are left out: [(RL, residue, [c, ..])]."""
    Hp = max(hyst, 1)
    out = []
    for RL in ROWS:
        for res in (RL - 1, 0):
            cs = [c for c in range(res, T, RL) if reachable(L, T, c - Hp)]
            if cs:
                k = _Lcg(L + T + hyst + RL + res).below(len(cs))
                out.append((RL, res, cs[k:] + cs[:k]))
    return out


def _has_close(ei, T, c):
    return len(ei) > 0 and bool(np.any((ei[:, 2] == c) & (c < T)))


@functools.lru_cache(maxsize=None)
def _gap_cached(L, T, g, alt):
    return gap_stream(L, T, g, unit(L, 11 + g + 1000 * alt), seed=L + 3 * T + 7 * g + 5 * alt)


@functools.lru_cache(maxsize=None)
def _fixed(L, T):
    """The streams that do not depend on the hysteresis: [(name, iq)]."""
    out = []
    u = unit(L, 1)
    z = np.zeros((T, 2), np.int16)
    out.append(("zero", z))
    s = np.zeros(T, np.int8)
    s[0] = 1
    if T > L:
        s[L] = 1
    out.append(("zero_head", samples(s, u)))
    out.append(("rot_j", samples(np.ones(T, np.int8), unit(L, 2), rot=1)))
    out.append(("rot_neg", samples(np.ones(T, np.int8), unit(L, 3), rot=2)))
    out.append(("never", pattern_stream(L, T, L, [], unit(L, 4))))
    g = _Lcg(L * 31 + T)
    for i, h in enumerate(_supports(L)):
        # plateaus: levels rise after the gate opens, and come back to the same maximum later
        a0 = amin(L, h) + 2 + g.below(8)
        pat = [1] * 3 + [0] * 2 + [2] * 4 + [1] * 5 + [2] * 3 + [0] * 3 + [1] * 130 + [2] * 2 + [1] * 20 + [2] * 3
        out.append((f"plateau{i}", pattern_stream(L, T, a0, pat, unit(L, 5 + i), h=h)))
    # many short gates: more than the event slots hold, for a small hysteresis
    h = ([q for q in _supports(L) if T - amin(L, q) >= 70] or [_supports(L)[-1]])[0]
    # single above samples at both parities of n: while the window fills v moves by +-1, and only
    # one parity of n can hold the lowest above value
    pat = ([1] + [0] * 3 + [1] + [0] * 4) * 30
    out.append(("many", pattern_stream(L, T, amin(L, h) + 9, pat, unit(L, 9), h=h)))
    pat = ([1] + [0] * 19 + [1] + [0] * 20) * 20
    out.append(("many19", pattern_stream(L, T, amin(L, h) + 9, pat, unit(L, 10), h=h)))
    return out


@functools.lru_cache(maxsize=None)
def streams1(L, T, hyst):
    """One-antenna set: (names, iq [B, T, 2] int16), B odd."""
    Hp = max(hyst, 1)
    named = list(_fixed(L, T))
    for g in (Hp - 1, Hp, Hp + 1):
        if g + 1 < T - L:
            for alt in (0, 1):                                # two positions of every gap
                iq = _gap_cached(L, T, g, alt)
                if iq is not None:
                    named.append((f"gap{g}{'b' if alt else ''}", iq))
    J = tuple(range(6))
    for RL, res, cs in close_targets(L, T, hyst):
        iq = pulse_stream(L, T, [c - Hp for c in cs], unit(L, 20 + res), hyst,
                          lambda ei, P, M, RL=RL, res=res: len(ei) > 0 and bool(np.any((ei[:, 2] < T) & (ei[:, 2] % RL == res))),
                          jits=J)
        if iq is not None:
            named.append((f"close{RL}_{res}", iq))
    ends = [("open_last", [T - 1], 1, lambda ei, P, M: len(ei) > 0 and ei[-1, 1] == T - 1),
            ("close_last", [T - 1 - Hp], 2, lambda ei, P, M: _has_close(ei, T, T - 1)),
            ("close_T", [T - Hp], 2, lambda ei, P, M: len(ei) > 0 and ei[-1, 2] == T and
             bool(M[min(max(T - Hp, 0), T - 1)] >= THR) and not bool(np.any(M[T - Hp + 1:] >= THR))),
            ("open_T", list(range(T - 3, T - 12, -1)), 2, lambda ei, P, M: len(ei) > 0 and ei[-1, 2] == T)]
    for name, ps, r, pred in ends:
        iq = pulse_stream(L, T, [p for p in ps if p > L], unit(L, 30 + r), hyst, pred, r=r, jits=J)
        if iq is not None:
            named.append((name, iq))
    if len(named) % 2 == 0:
        named.append(("never2", pattern_stream(L, T, L, [], unit(L, 40))))
    names = tuple(n for n, _ in named)
    iq = np.stack([q for _, q in named])
    iq.setflags(write=False)
    return names, iq


@functools.lru_cache(maxsize=None)
def streams(L, T, hyst, n_ant=1):
    """(names, iq [B, n_ant, T, 2] int16).  Two antennas: the second is zero (b % 3 == 0), j times
    the first (b % 3 == 1) or another stream of the set (b % 3 == 2; a zero second antenna where
    either P is not real: the sum must stay on an axis)."""
    names, iq = streams1(L, T, hyst)
    if n_ant == 1:
        return names, iq[:, None]
    B = len(names)
    out = np.zeros((B, 2, T, 2), np.int16)
    out[:, 0] = iq
    for b in range(B):
        other = (b + 5) % B
        if b % 3 == 1:
            out[b, 1, :, 0], out[b, 1, :, 1] = -iq[b, :, 1], iq[b, :, 0]
        elif b % 3 == 2 and not names[b].startswith("rot") and not names[other].startswith("rot"):
            out[b, 1] = iq[other]
            M = O.aa_metric(cplx(out[b]), L)[2]              # v0 + v1 over r0 + r1: any ratio
            if T > L and np.min(np.abs(M[L:] - THR)) < 2 * MARGIN:
                out[b, 1] = 0
    out.setflags(write=False)
    return names, out


@functools.lru_cache(maxsize=None)
def oracle(L, T, hyst, n_ant=1):
    """[(P, R, M, valid, ev_int, ev_real)] per stream of streams(L, T, hyst, n_ant)."""
    _, iq = streams(L, T, hyst, n_ant)
    return [O.aa_detect(cplx(iq[b]), L, THR, hyst, FS) for b in range(iq.shape[0])]


# ------------------------------------------------------------------------------------------------
# preconditions and coverage
# ------------------------------------------------------------------------------------------------
def below_gaps(M, L):
    idx = np.flatnonzero(M[L:] >= THR)
    return set((np.diff(idx) - 1).tolist())


def tie_kinds(P, ei, E_lane=2, row=128):
    """Which kinds of tie pairs (p1 < p2, both at the gate's maximum |P|^2) the gates hold."""
    kinds = set()
    pm = np.abs(P) ** 2
    T = len(P)
    for peak, start, end, _ in ei:
        seg = pm[start:min(end, T - 1) + 1]
        at = start + np.flatnonzero(seg == seg.max())
        if len(at) < 2:
            continue
        p1 = at[0]
        assert p1 == peak
        for p2 in at[1:]:
            if p2 == p1 + 1 and p1 % E_lane == 0:
                kinds.add("lane")
            elif p2 // row == p1 // row and p2 // E_lane != p1 // E_lane:
                kinds.add("row")
            elif p2 // row != p1 // row:
                kinds.add("rows")
    return kinds


def expected_coverage(L, T, hyst):
    """The coverage conditions that apply to a shape, by what a stream of length T can hold at all.
    The first sample a built stream can have above the threshold is a0 = amin(L, 32) (support of 32
    phases); the zero-head stream is above on L .. 2L - 1.

    gaps: Hp - 1, Hp, Hp + 1 between above samples where Hp + 1 < T - L and some support can hold
    both above samples (gap_fits);
    closes: per (RL, residue) where some c < T of that residue has a reachable c - Hp;
    open_L: T > L;  open_last / close_last / close_T: where the above sample is reachable;
    ties, peak_later, overflow: where T - a0 holds the patterns (T - L >= 300 and, for the overflow,
    five gates and their hysteresis)."""
    Hp = max(hyst, 1)
    a0 = amin(L, 32) + 1
    cov = {"gaps": [g for g in (Hp - 1, Hp, Hp + 1) if Hp + 1 < T - L and gap_fits(L, T, g)],
           "closes": [(RL, res) for RL, res, _ in close_targets(L, T, hyst)],
           "open_L": T > L,
           "open_last": reachable(L, T, T - 1),
           "close_last": reachable(L, T, T - 1 - Hp),
           "close_T": reachable(L, T, T - Hp),
           "ties": T - L >= 300,
           "peak_later": T - L >= 300,
           "overflow": T - a0 >= (MAX_EVENTS + 1) * (Hp + 3) + 40 and Hp <= 19}
    return cov


def check(L, T, hyst, n_ant=1):
    """Preconditions on the oracle's output of streams(L, T, hyst, n_ant) and, for one antenna, the
    coverage of the gate machine's edges; returns the coverage found (dict)."""
    names, iq = streams(L, T, hyst, n_ant)
    B = iq.shape[0]
    assert B % 2 == 1
    Hp = max(hyst, 1)
    orc = oracle(L, T, hyst, n_ant)
    gaps, closes, ties = set(), set(), set()
    found = dict(open_L=False, open_last=False, close_last=False, close_T=False, peak_later=False, overflow=False)
    margin = 1.0
    for b in range(B):
        P, R, M, valid, ei, er = orc[b]
        x = cplx(iq[b])
        assert np.array_equal(P.real, np.rint(P.real)) and np.array_equal(P.imag, np.rint(P.imag)), names[b]
        assert np.array_equal(R, np.rint(R)), names[b]
        assert not np.any(P.real * P.imag), names[b]
        assert np.max(np.abs(P) ** 2, initial=0) <= 2 ** 24, names[b]
        prod = np.zeros_like(x)
        prod[:, L:] = x[:, L:] * np.conj(x[:, :-L])
        pre = np.cumsum(prod.sum(0))
        assert max(np.max(np.abs(pre.real), initial=0), np.max(np.abs(pre.imag), initial=0),
                   float(np.sum(np.abs(x) ** 2))) < 2 ** 24, names[b]
        if T > L:
            margin = min(margin, float(np.min(np.abs(M[L:] - THR))))
        assert not np.any(np.isnan(M))
        if n_ant != 1:
            continue
        gaps |= below_gaps(M, L)
        for peak, start, end, _ in ei:
            if end < T:
                closes |= {(RL, end % RL) for RL in ROWS}
            found["open_L"] |= start == L
            found["open_last"] |= start == T - 1
            found["close_last"] |= end == T - 1
            found["peak_later"] |= peak != start
        if len(ei) and ei[-1, 2] == T:
            found["close_T"] = True
        found["overflow"] |= len(ei) > MAX_EVENTS
        ties |= tie_kinds(P, ei)
    assert margin >= MARGIN, margin
    if n_ant != 1:
        return dict(margin=margin)
    want = expected_coverage(L, T, hyst)
    for g in want["gaps"]:
        assert g in gaps, ("gap", g, L, T, hyst)
    for RL, res in want["closes"]:
        assert (RL, res) in closes, ("close", RL, res, L, T, hyst)
    for k in ("open_L", "open_last", "close_last", "close_T", "peak_later", "overflow"):
        if want[k]:
            assert found[k], (k, L, T, hyst)
    if want["ties"]:
        assert ties >= {"lane", "row", "rows"}, (ties, L, T, hyst)
    return dict(margin=margin, gaps=sorted(g for g in gaps if g in (Hp - 1, Hp, Hp + 1)), closes=sorted(closes & {
        (RL, r) for RL in ROWS for r in (RL - 1, 0)}), ties=sorted(ties), **found)
