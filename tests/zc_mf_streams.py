"""Exact streams for the ZC matched filter and its normaliser (test infrastructure, host only).

The matched filter corr[n] = Σ_j xz[n-N+1+j]·conj(ref[j]) (zc_v2.py:244-254) and the window energy
Σ |xz|² over the same N samples (zc_v2.py:266-268) are sums of products.  With integer-valued samples
and integer-valued taps every product and every partial sum is an integer below 2^53 (facts(), asserted by
tests/test_zc_mf_streams_host.py), so

  * the direct kernel (corr.hip zc_mf_kernel: fp64 FMA chains) is EXACT, in any summation order;
  * the overlap-save kernels' energy prefix (zc_fftcorr.hip) is exact too, and their only error is
    the block FFT's, bounded per block by model 4 of tests/error_models.py.

The expectations here come from integers alone: four int64 convolutions for corr, one int64
convolution of |x|² with ones per branch for the energy; the normalised modes are then evaluated in
np.longdouble (64-bit mantissa: 2^-11 of a float64 ulp) from those integers and the float64
ref_energy the C ABI is given (np.sum(np.abs(ref)**2), as the reference computes it).  Nothing is
taken from the float64 oracle.

Streams (components fit int16, so one stream serves int16, c64 and c128):
  noise     components in [-3, 3] everywhere
  zero      noise with an all-zero span of N + 252 samples: window energy exactly 0 inside, so the V2
            clamp max(e, 1e-12) and the COMBINED +1e-12 decide the output
  loud      noise with a 64-sample burst of amplitude ~3e4 at 9000 (N = 2048: inside the block whose
            input span is [4098, 12290) and no other), so one block is loud and its neighbours quiet
  straddle  c128 only, every sample scaled by 2^-21 (exact): isolated samples of magnitude 1 or 2 so
            that N-sample windows hold Σk² of 0, 1, 4, 5 or 8; 4·2^-42 = 9.09e-13 and 5·2^-42 =
            1.137e-12 straddle the 1e-12 of max(e, 1e-12)
  inexact   c128 only: 16 samples of 2^27 next to noise in one block, so the fp64 energy prefix of the
            overlap-save kernels is no longer exact (model |d e| <= k_e·u·E_block); corr stays exact
  huge      c128 only: noise·2^654 (|corr| up to 9e199, exact); |x|² overflows fp64
Lengths for N = 2048 (M = 8192, S = 6145): 10243 (nout = 2S), 10244 (nout = 2S + 1: the last block has
one output), 16384 (three blocks), 1000 (shorter than the reference), 1; for N = 256 and 300: 3000.

check(stream, ...) is the one checker: the GPU tests (tests/test_gpu_zc_mf_exact.py) and the host
proof (tests/test_zc_mf_streams_host.py, which feeds it mutants of the numpy model below) both call it.
It skips no output.  The numpy fp64 overlap-save model os_model() passes it at 4e-6 to 2.5e-5 of the
per-block bound (printed by the host proof; 0.012 of u·log2(M)·||u_q||·||ref|| on the 3-block noise stream,
0.066 the worst of all cases).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import error_models as EM

LD = np.longdouble
U = 2.0 ** -53
A = 3
RAW, V2, COMBINED, NORMALIZE, SUM = 0, 1, 2, 3, 4           # OFS_ZC_* (include/ofdmsync.h)
MODE_NAME = {RAW: "raw", V2: "v2", COMBINED: "combined", NORMALIZE: "v2", SUM: "sum"}
N_BIG, M_BIG = 2048, 8192
S_BIG = M_BIG - N_BIG + 1
LENGTHS_BIG = (10243, 10244, 16384, 1000, 1)
EXACT_SLACK = 2.0 ** -8      # units of u: the longdouble expectation's own error (a few 2^-64 relative)


def pick_m(N: int, T: int, nb: int) -> int:
    """The block length the tests plan with: 8192 for 2048 taps (the only length the fused and the
    persistent kernel take), else the smallest-work power of two as zc_fftcorr.hip pick_m chooses."""
    if N == N_BIG:
        return M_BIG
    nout, best, cost = T + N - 1, 0, None
    for lg in range(10, 17):
        M = 1 << lg
        if M < 2 * N or (nb * (M + 1025) + 16) * 8 > 160 * 1024:
            continue
        S = M - N + 1
        c = -(-nout // S) * M
        if cost is None or c < cost:
            best, cost = M, c
    return best


@functools.lru_cache(maxsize=None)
def taps(N: int):
    """Gaussian-integer taps (re, im), components in [-3, 3], not all zero."""
    r = np.random.default_rng(1000 + N).integers(-A, A + 1, (2, N))
    r[0, 0] = 2
    r.setflags(write=False)
    return r


def ref_c(N: int) -> np.ndarray:
    r = taps(N)
    return (r[0] + 1j * r[1]).astype(np.complex128)


def ref_energy(N: int) -> float:
    """The scalar the C ABI is given: as zc_v2.py:263 and correlate_batched compute it."""
    return float(np.sum(np.abs(ref_c(N)) ** 2))


class Stream:
    """Integer samples xr + i·xi [nb, T], all scaled by 2^shift; the exact integer corr and energy."""

    def __init__(self, name, N, xr, xi, shift=0):
        self.name, self.N, self.shift = name, int(N), int(shift)
        self.xr = np.ascontiguousarray(xr, np.int64)
        self.xi = np.ascontiguousarray(xi, np.int64)
        self.xr.setflags(write=False)
        self.xi.setflags(write=False)
        self.nbmax, self.T = self.xr.shape
        self.nout = self.T + self.N - 1
        self._exact = None

    def x(self, nb: int, fmt: str) -> np.ndarray:
        """[nb, T] complex (c64 / c128) or [nb, T, 2] int16."""
        if fmt == "int16":
            assert self.shift == 0 and max(np.abs(self.xr).max(), np.abs(self.xi).max()) <= 32767
            return np.stack([self.xr[:nb], self.xi[:nb]], -1).astype(np.int16)
        z = np.ldexp(self.xr[:nb].astype(np.float64), self.shift) + 1j * np.ldexp(self.xi[:nb].astype(np.float64), self.shift)
        if fmt == "c64":
            assert self.shift == 0 and max(np.abs(self.xr).max(), np.abs(self.xi).max()) < 2 ** 24
            return z.astype(np.complex64)
        return z

    def exact(self):
        """(cr, ci, e) int64 [nbmax, nout]: corr = (cr + i·ci)·2^shift, window energy e·2^(2·shift)."""
        if self._exact is None:
            rr, ri = taps(self.N)
            hr, hi = rr[::-1].astype(np.int64), -ri[::-1].astype(np.int64)     # h = conj(ref reversed)
            one = np.ones(self.N, np.int64)
            cr, ci, e = [], [], []
            for a, b in zip(self.xr, self.xi):
                cr.append(np.convolve(a, hr) - np.convolve(b, hi))
                ci.append(np.convolve(a, hi) + np.convolve(b, hr))
                e.append(np.convolve(a * a + b * b, one))
            self._exact = tuple(np.stack(v) for v in (cr, ci, e))
            for v in self._exact:
                v.setflags(write=False)
        return self._exact

    def partial_sum_bound(self) -> int:
        """An upper bound of every partial sum of corr's components and of the energy, in any order."""
        rr, ri = taps(self.N)
        h = (np.abs(rr) + np.abs(ri))[::-1].astype(np.int64)
        m = 0
        for a, b in zip(self.xr, self.xi):
            m = max(m, int(np.convolve(np.abs(a) + np.abs(b), h).max()),
                    int(np.convolve(a * a + b * b, np.ones(self.N, np.int64)).max()))
        return m

    def block_norms(self, M: int):
        """||u_q||_2 (longdouble, scaled) [nbmax, nblk] and the block energies' integers [nbmax, nblk]."""
        S = M - self.N + 1
        nblk = -(-self.nout // S)
        e = np.zeros((self.nbmax, (nblk - 1) * S + M), np.int64)
        e[:, self.N - 1:self.N - 1 + self.T] = self.xr * self.xr + self.xi * self.xi
        Eb = np.stack([e[:, q * S:q * S + M].sum(axis=1) for q in range(nblk)], axis=1)
        return np.ldexp(np.sqrt(Eb.astype(LD)), self.shift), Eb


NBMAX = 3
ZERO_EXTRA = 252
LOUD_AT, LOUD_LEN = 9000, 64


def _noise(rng, T):
    return rng.integers(-A, A + 1, (NBMAX, T)), rng.integers(-A, A + 1, (NBMAX, T))


def zero_span(N: int, T: int):
    """[start, stop) of the zero family's all-zero span: its zero-energy outputs lie across a block seam
    (6145 for N = 2048; 1793 / 1749 for N = 256 / 300 in 2048-sample blocks)."""
    s0 = 4000 if N == N_BIG else 1400
    return s0, s0 + N + ZERO_EXTRA


@functools.lru_cache(maxsize=None)
def stream(family: str, N: int, T: int) -> Stream:
    rng = np.random.default_rng(N * 100003 + T * 17 + len(family))
    xr, xi = _noise(rng, T)
    shift = 0
    if family == "zero":
        a, b = zero_span(N, T)
        assert b + N < T
        xr[:, a:b] = 0
        xi[:, a:b] = 0
    elif family == "loud":
        at = LOUD_AT if N == N_BIG else 2000
        assert at + LOUD_LEN <= T
        sg = rng.choice([-1, 1], (2, NBMAX, LOUD_LEN))
        xr[:, at:at + LOUD_LEN] = sg[0] * rng.integers(29000, 32768, (NBMAX, LOUD_LEN))
        xi[:, at:at + LOUD_LEN] = sg[1] * rng.integers(29000, 32768, (NBMAX, LOUD_LEN))
    elif family == "straddle":
        xr[:], xi[:] = 0, 0
        shift = -21
        # branch 0: windows hold 1 | 4 | 4, 5, 1 | 4, 8, 4; branch 1 the same content 100 samples later
        for br, off in ((0, 0), (1, 100), (2, 333)):
            for pos, (re, im) in ((100, (1, 0)), (2500, (0, 2)), (5000, (2, 0)), (5700, (0, -1)), (8000, (-2, 0)),
                                  (8900, (0, 2))):
                xr[br, pos + off], xi[br, pos + off] = re, im
    elif family == "inexact":
        xr[:, 7000:7016] = 2 ** 27
        xi[:, 7000:7016] = 0
    elif family == "huge":
        shift = 654
    else:
        assert family == "noise", family
    return Stream(f"{family}_N{N}_T{T}", N, xr, xi, shift)


FAMILIES = ("noise", "zero", "loud")


def cases():
    """(family, N, T) of the integer streams every format runs: the three families at the three long
    lengths and at N = 256 / 300, noise alone at the two lengths that hold nothing else."""
    out = [(f, N_BIG, T) for T in LENGTHS_BIG[:3] for f in FAMILIES]
    out += [("noise", N_BIG, 1000), ("noise", N_BIG, 1)]
    out += [(f, N, 3000) for N in (256, 300) for f in FAMILIES]
    return out


# ---------------------------------------------------------------------------------------------
# exact expectations
# ---------------------------------------------------------------------------------------------
class Expected:
    """Per output row r and branch term t: value Σ_t c[r, t]·w[r, t] with the exact complex c (re, im) and
    the exact real weight w (1 in RAW / SUM, 1 / (|ref|·sqrt(clamped energy)) in the normalised modes)."""

    def __init__(self, cre, cim, w, e, mode):
        self.cre, self.cim, self.w, self.e, self.mode = cre, cim, w, e, mode
        self.re, self.im = (cre * w).sum(axis=1), (cim * w).sum(axis=1)
        self.are, self.aim = np.abs(cre * w).sum(axis=1), np.abs(cim * w).sum(axis=1)
        self.mag = np.sqrt(self.re * self.re + self.im * self.im)


def clamp_weight(e, mode, rn):
    """w = 1 / (rn·sqrt(clamped energy)) of the normalised modes, e [terms, nout] longdouble."""
    if mode == COMBINED:
        ew = np.maximum(e.sum(axis=0, keepdims=True), LD(0)) + LD(1e-12)            # zc.py:113-126
        ew = np.broadcast_to(ew, e.shape)
    else:
        ew = np.maximum(e, LD(1e-12))                                               # zc_v2.py:268
    return 1 / (rn * np.sqrt(ew))


def expected(st: Stream, nb: int, mode: int, shift_by: int = 0, rot: int = 0) -> Expected:
    """The exact outputs of `mode` over the first nb branches (NORMALIZE: branch 0), optionally of the
    stream delayed by shift_by samples and multiplied by i^rot (the many-block batch)."""
    cr, ci, e = st.exact()
    if mode == NORMALIZE:
        nb = 1
    cr, ci, e = cr[:nb], ci[:nb], e[:nb]
    if shift_by:
        assert not cr[:, st.nout - shift_by:].any() and not e[:, st.nout - shift_by:].any()
        z = np.zeros((nb, shift_by), np.int64)
        cr, ci, e = (np.concatenate([z, v[:, :st.nout - shift_by]], axis=1) for v in (cr, ci, e))
    for _ in range(rot % 4):
        cr, ci = -ci, cr
    cre, cim = np.ldexp(cr.astype(LD), st.shift), np.ldexp(ci.astype(LD), st.shift)
    el = np.ldexp(e.astype(LD), 2 * st.shift)
    if mode in (RAW, SUM):
        w = np.ones_like(cre)
    else:
        w = clamp_weight(el, mode, np.sqrt(LD(ref_energy(st.N))))
    if mode == RAW:
        return Expected(cre[:, None], cim[:, None], w[:, None], el[:, None], mode)
    return Expected(cre[None], cim[None], w[None], el[None], mode)


# ---------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------
class Verdict:
    def __init__(self):
        self.ok, self.why = True, []
        self.ratio = 0.0            # largest |error| / bound over corr and |corr| (bounds > 0)
        self.block_ratio = None     # per block: largest corr ratio (overlap-save kernels)
        self.ulps = 0.0             # largest component error in float64 ulps of the exact value
        self.n_checked = 0

    def fail(self, msg):
        self.ok = False
        self.why.append(msg)

    def __bool__(self):
        return self.ok


def _ratio(err, bound):
    """max err / bound with 0 / 0 = 0 and anything above a zero bound = inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bound)
    r = np.where(np.isnan(r), LD(np.inf), r)
    return r


def check(st: Stream, nb: int, mode: int, corr, mag, kernel: str, M: int = 0, ke: float = 0.0,
          exp: Expected | None = None) -> Verdict:
    """Every output of corr (complex [rows, nout]) and mag ([rows, nout], either may be None) against the exact
    expectation.  kernel "direct": RAW / SUM bit for bit and |corr| within 1 ulp of the correctly rounded root,
    the normalised modes within zc_norm_k("div") roundings.  kernel "pers" / "fused" / "rocfft" / "numpy"
    with block length M: the per-block bound of error model 4 on corr, propagated through the exact window
    energy (ke > 0: through the energy model |d e| <= ke·u·E_block) plus the counted roundings of that
    kernel's normaliser (one branch: its fused extract; more: mc_extract_kernel's "div" sequence)."""
    v = Verdict()
    ex = exp if exp is not None else expected(st, nb, mode)
    rows, nterm, nout = ex.cre.shape
    name = MODE_NAME[mode]
    seq = "div" if kernel in ("direct", "rocfft", "numpy") or nterm > 1 or (mode == RAW and nb > 1) else kernel
    k, kmag = EM.zc_norm_k(seq, name, nterm)
    slack = 0.0 if name in ("raw", "sum") else EXACT_SLACK
    bfft = np.zeros(ex.cre.shape, LD)
    if kernel != "direct":
        S = M - st.N + 1
        un, Eb = st.block_norms(M)
        bq = EM.zc_os_block_bound(un, ref_c(st.N), M, kernel)                       # [nbmax, nblk]
        per_out = np.repeat(bq, S, axis=1)[:, :nout]
        bfft = (per_out[:rows * nterm].reshape(rows, nterm, nout) if mode == RAW else per_out[None, :nterm]).astype(LD)
    w, are, aim = ex.w, ex.are, ex.aim
    ext_re = ext_im = LD(0)
    if ke and name not in ("raw", "sum"):
        # the window energy anywhere in [e - de, e + de]: the weight at most wlo = w(e - de), which scales
        # every term (and the FFT's share) by at most wlo / w
        de = np.repeat(ke * U * np.ldexp(Eb.astype(LD), 2 * st.shift), S, axis=1)[:, :nout][None, :nterm]
        wlo = clamp_weight((ex.e - de)[0], mode, np.sqrt(LD(ref_energy(st.N))))[None]
        ext_re = (np.abs(ex.cre) * (wlo - w)).sum(axis=1)
        ext_im = (np.abs(ex.cim) * (wlo - w)).sum(axis=1)
        are, aim = (np.abs(ex.cre) * wlo).sum(axis=1), (np.abs(ex.cim) * wlo).sum(axis=1)
        w = wlo
    bound_abs = (bfft * w).sum(axis=1)
    bre = bound_abs + ext_re + (k + slack) * U * are
    bim = bound_abs + ext_im + (k + slack) * U * aim
    if corr is not None:
        corr = np.asarray(corr).reshape(rows, nout)
        gre, gim = corr.real.astype(LD), corr.imag.astype(LD)
        if not (np.isfinite(corr.real).all() and np.isfinite(corr.imag).all()):
            v.fail("non-finite corr")
            return v
        ere, eim = np.abs(gre - ex.re), np.abs(gim - ex.im)
        r = np.maximum(_ratio(ere, bre), _ratio(eim, bim))
        v.n_checked += r.size
        v.ratio = max(v.ratio, float(r.max()))
        if kernel != "direct":
            S = M - st.N + 1
            pad = (-nout) % S
            rb = np.concatenate([r.max(axis=0), np.zeros(pad, LD)]).reshape(-1, S).max(axis=1)
            v.block_ratio = rb.astype(np.float64)
        if kernel == "direct" and name in ("raw", "sum"):
            if (ere != 0).any() or (eim != 0).any():
                i = np.argwhere((ere != 0) | (eim != 0))[0]
                v.fail(f"corr differs from the exact integers, first at {tuple(i)}")
            if (np.signbit(corr.real) & (corr.real == 0)).any() or (np.signbit(corr.imag) & (corr.imag == 0)).any():
                v.fail("-0.0 where the exact sum is 0")
        elif not (r <= 1).all():
            i = np.unravel_index(int(np.argmax(r)), r.shape)
            v.fail(f"corr outside the bound at {i}: ratio {float(r[i]):.3g}")
        with np.errstate(divide="ignore", invalid="ignore"):
            for g, e_ in ((corr.real, ex.re), (corr.imag, ex.im)):
                sp = np.spacing(np.abs(e_.astype(np.float64)))
                u_ = np.where(e_ == 0, 0.0, (np.abs(g.astype(LD) - e_) / np.where(e_ == 0, 1.0, sp)).astype(np.float64))
                v.ulps = max(v.ulps, float(np.max(u_)))
    if mag is not None:
        mag = np.asarray(mag).reshape(rows, nout)
        if not np.isfinite(mag).all():
            v.fail("non-finite |corr|")
            return v
        if kernel == "direct" and name in ("raw", "sum"):
            cr_ = ex.mag.astype(np.float64)                                 # the correctly rounded root
            r = _ratio(np.abs(mag - cr_).astype(LD), np.spacing(cr_).astype(LD))
        else:
            bm = np.sqrt(bre * bre + bim * bim) + (kmag + slack) * U * ex.mag
            r = _ratio(np.abs(mag.astype(LD) - ex.mag), bm)
        v.n_checked += r.size
        v.ratio = max(v.ratio, float(r.max()))
        if not (r <= 1).all():
            i = np.unravel_index(int(np.argmax(r)), r.shape)
            v.fail(f"|corr| outside the bound at {i}: ratio {float(r[i]):.3g}")
        if (mag < 0).any() or (np.signbit(mag) & (mag == 0)).any():
            v.fail("negative |corr|")
    return v


def old_criterion(corr, mag, exp: Expected) -> bool:
    """What tests/test_gpu_corr.py::test_zc_fft_overlap_save_equals_direct asks today, against the exact
    value in place of the direct kernel: corr within 1e-11 of the row maximum, |corr| rtol 1e-9 plus
    1e-11 of the largest row maximum."""
    ref = (exp.re + 1j * exp.im).astype(np.complex128)
    scale = np.abs(ref).max(axis=-1, keepdims=True)
    if not np.max(np.abs(np.asarray(corr).reshape(ref.shape) - ref) / scale) < 1e-11:
        return False
    m = np.asarray(mag).reshape(ref.shape)
    return bool(np.all(np.abs(m - np.abs(ref)) <= 1e-11 * float(scale.max()) + 1e-9 * np.abs(ref)))


# ---------------------------------------------------------------------------------------------
# the numpy fp64 overlap-save model and its mutants
# ---------------------------------------------------------------------------------------------
MUTANTS = ("shift_one", "neighbour_block", "off_by_one_raw", "energy_n_minus_1", "energy_n_plus_1", "no_conj",
           "taps_not_reversed", "branch1_ignored", "v2_combined_swapped", "quiet_block_1e-9")
GAP_MUTANT = "quiet_block_5e-12"     # inside the present criterion, outside the per-block one (loud family)


def quiet_block(st: Stream, M: int) -> int:
    """The block with the smallest input energy among those with outputs (ties: the first)."""
    _, Eb = st.block_norms(M)
    return int(np.argmin(Eb[0]))


def os_model(st: Stream, nb: int, mode: int, M: int, mut: str | None = None):
    """(corr, mag) of numpy's fp64 FFT overlap-save with the reference's float64 normaliser; `mut` makes
    one of the errors of MUTANTS."""
    N, T, nout = st.N, st.T, st.nout
    S = M - N + 1
    nblk = -(-nout // S)
    ref = ref_c(N)
    h = np.conj(ref[::-1])
    if mut == "no_conj":
        h = ref[::-1].copy()
    elif mut == "taps_not_reversed":
        h = np.conj(ref)
    H = np.fft.fft(h, M)
    x = st.x(nb, "c128")
    if mut == "branch1_ignored":
        x = x.copy()
        x[1:2] = 0
    xp = np.zeros((nb, (nblk - 1) * S + M), np.complex128)
    xp[:, N - 1:N - 1 + T] = x
    blocks = [np.fft.ifft(np.fft.fft(xp[:, q * S:q * S + M], axis=1) * H, axis=1)[:, N - 1:] for q in range(nblk)]
    if mut == "neighbour_block":
        q = 1 if nblk > 1 else 0
        blocks[q] = blocks[q - 1] if nblk > 1 else blocks[q][:, ::-1]
    c = np.concatenate(blocks, axis=1)[:, :nout]
    W = N - 1 if mut == "energy_n_minus_1" else N + 1 if mut == "energy_n_plus_1" else N
    e2 = np.ldexp((st.xr[:nb] ** 2 + st.xi[:nb] ** 2).astype(np.float64), 2 * st.shift)
    if mut == "branch1_ignored":
        e2[1:2] = 0
    e = np.stack([np.concatenate([np.convolve(r, np.ones(W)), [0.0]])[:nout] for r in e2])   # the W samples ending at n
    rn = np.sqrt(ref_energy(N))
    m = mode
    if mut == "v2_combined_swapped":
        m = {V2: COMBINED, COMBINED: V2}.get(mode, mode)
    if m == RAW:
        out = c
    elif m == SUM:
        out = c.sum(axis=0, keepdims=True)
    elif m == COMBINED:
        out = (c.sum(axis=0) / (rn * np.sqrt(np.maximum(e.sum(axis=0), 0.0) + 1e-12)))[None]
    else:
        out = (c / (rn * np.sqrt(np.maximum(e, 1e-12)))).sum(axis=0, keepdims=True)
    out = np.array(out)
    if mut == "shift_one":
        out = np.roll(out, 1, axis=1)
    if mut == "off_by_one_raw" and mode == RAW:
        out[0, min(nout - 1, S + 7)] += math.ldexp(1.0, st.shift)
    if mut in ("quiet_block_1e-9", GAP_MUTANT):
        q = quiet_block(st, M)
        n = min(q * S + S // 2, nout - 1) if q * S < nout else nout - 1
        out[0, n] += float(mut.split("_")[-1]) * np.abs(out[0]).max()
    return out, np.hypot(out.real, out.imag)        # (np.abs of a complex array is 2 ulp off in places)


# ---------------------------------------------------------------------------------------------
# the many-block batch
# ---------------------------------------------------------------------------------------------
BATCH_B, BATCH_T = 180, 16384
BATCH_DMAX = 4200
# delays that move the bases' content (the burst at 6000: before, up to, across and past the output seam at
# 6145 and the start of the third block's input span at 10243; the zero span; both ends of the content)
BATCH_DELAYS = (0, 1, 2, 3, 81, 82, 144, 145, 146, 512, 1023, 2047, 2048, 2049, 3000, 4097, 4098, 4099, 4179, 4180,
                BATCH_DMAX)
BATCH_BURST_AT = 6000


@functools.lru_cache(maxsize=None)
def batch_bases():
    """Three base streams of BATCH_T samples whose last BATCH_DMAX samples are zero: noise, noise with a zero
    span, noise with a loud burst across the first seam."""
    rng = np.random.default_rng(20260)
    Lc = BATCH_T - BATCH_DMAX
    out = []
    for fam in FAMILIES:
        xr, xi = (v[:1] for v in _noise(rng, BATCH_T))
        xr[:, Lc:], xi[:, Lc:] = 0, 0
        if fam == "zero":
            xr[:, 5000:5000 + N_BIG + ZERO_EXTRA], xi[:, 5000:5000 + N_BIG + ZERO_EXTRA] = 0, 0
        if fam == "loud":
            xr[:, BATCH_BURST_AT:BATCH_BURST_AT + LOUD_LEN] = rng.integers(29000, 32768, LOUD_LEN)
            xi[:, BATCH_BURST_AT:BATCH_BURST_AT + LOUD_LEN] = -rng.integers(29000, 32768, LOUD_LEN)
        out.append(Stream("batch_" + fam, N_BIG, xr, xi))
    return tuple(out)


def batch_plan():
    """(base index, delay, rotation) of stream b."""
    return [(b % 3, BATCH_DELAYS[(b // 3 + 5 * (b % 3)) % len(BATCH_DELAYS)], b % 4) for b in range(BATCH_B)]


def batch_stream(b: int) -> Stream:
    """Stream b of the batch as a Stream of its own (exact() is NOT to be called on it: use batch_expected)."""
    k, d, rot = batch_plan()[b]
    base = batch_bases()[k]
    xr, xi = np.zeros((1, BATCH_T), np.int64), np.zeros((1, BATCH_T), np.int64)
    xr[:, d:], xi[:, d:] = base.xr[:, :BATCH_T - d], base.xi[:, :BATCH_T - d]
    for _ in range(rot):
        xr, xi = -xi, xr
    return Stream(f"batch{b}", N_BIG, xr, xi)


@functools.lru_cache(maxsize=None)
def batch_x() -> np.ndarray:
    """[BATCH_B, 1, BATCH_T] complex128 (integer components)."""
    x = np.stack([batch_stream(b).x(1, "c128") for b in range(BATCH_B)])
    x.setflags(write=False)
    return x


def batch_expected(b: int, mode: int) -> Expected:
    k, d, rot = batch_plan()[b]
    return expected(batch_bases()[k], 1, mode, shift_by=d, rot=rot)


def blocks_holding(sample: int, N: int, M: int, nout: int):
    """The overlap-save blocks whose input span [q·S - (N-1), q·S - (N-1) + M) holds `sample`."""
    S = M - N + 1
    return [q for q in range(-(-nout // S)) if q * S - (N - 1) <= sample < q * S - (N - 1) + M]


# ---------------------------------------------------------------------------------------------
# preconditions (host proof)
# ---------------------------------------------------------------------------------------------
def facts(st: Stream):
    """What the stream holds: largest partial sum, the window-energy integers present, zero-energy outputs."""
    _, _, e = st.exact()
    return dict(partial=st.partial_sum_bound(), energies=set(np.unique(e[0]).tolist()) if st.shift == -21 else None,
                zero_windows=int((e[0][st.N - 1:st.T] == 0).sum()))
