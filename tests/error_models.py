"""fp32 error models of the engine's single-precision fast paths (test infrastructure).

Every fp32 parity test derives its tolerance from one of these models instead of a fixed
number, and prints the measured error next to the bound.  u = 2^-24 is the fp32 unit roundoff;
inputs are complex64 on both sides (the oracle promotes the same samples to fp64), so input
rounding is not an error source.

1. Window sums (win_fast.hip, sc_minn_pk_kernel: S&C / combined S&C / Minn; E samples per lane,
   NB branches).  A window sum S = wh + (xh + f[e]) + suffix is built from: the lagged products
   in fp32 (2u per component, NB branches accumulated: NB - 1 more adds), in-lane forward /
   backward partials (at most E - 1 adds), the fp64 lane scan and row totals (exact to fp32
   resolution) rounded to fp32 three times (in-row prefix, row remainder, rows inside the
   window), the retained suffix (1 add) and the final 3 adds.  Per real component
   |dS| <= (E + 8 + NB)·u·Σ|terms|, so for the complex P
       |dP| <= kP·u·S_abs + u·|P|,   kP = sqrt(2)·(E + 8 + NB),   S_abs = Σ |x_i|·|x_i+lag|,
   R (non-negative terms, up to 4 windows added): |dR| <= kR·u·R, kR = E + 11 + NB,
   and the metric M = c²/R² (c = |P| or max(Re P, 0); fma, mul, v_rcp_f32 1 ulp, mul):
       |dM| <= 2·(c/R)·(bP/R) + (bP/R)² + 2·M·bR/R + kM·u·M,   kM = 6.
   For combined S&C, S_abs <= R/2 (Cauchy-Schwarz) and M <= 1/4, so the bound is below
   (sqrt(M)·kP/2 + 2M·kR + kM·M)·u <= 5e-7 at E = 4: the north-star 1e-6 holds for every input.
2. FFT-based zc_freq metric (zc_win kernels: fp32 radix-2 column FFTs of R = N/64 points with
   fp32-rounded twiddles, then fp64 twiddled column sums per bin; rocFFT leg: an fp32 FFT of all
   log2(N) stages).  Normwise relative FFT error (Higham, Accuracy and Stability of Numerical
   Algorithms, Thm 24.2): eps <= stages·eta, eta = mu + gamma_4·(sqrt(2) + mu) ~ (1 + 4·sqrt(2))·u
   with mu = u the twiddle error.  The column sums in fp64 add no fp32 error; 2 stages are added
   for the fp32 products / gather.  With rho = ||db||/||b|| <= eps·sqrt(N)·||w||/||b|| (Parseval)
   and m = |<T, b>|²/(E_t·||b||²) over the nb·62 gathered bins:
       |dm| <= 2·(sqrt(nb·m) + m)·rho + (nb + 1)·rho² + kM·u·m.
   (oracle_zc_freq_check evaluates it per window from the fp64 bins.)
3. Park fp32 (corr.hip park_kernel<fp32>): every output's P(d) = Σ_br Σ_{k<N/2} x[d-k]·x[d+k] is one
   fp32 chain of 2 FMAs per term and component (park_mac), so per component
   |dP| <= gamma_{2·h·nb}·Σ (|b.x f.x| + |b.y f.y|) <= 2·h·nb·u·S_abs (Higham Eq. 3.5, first order;
   |b.x f.x| + |b.y f.y| <= |b|·|f|), h = N/2, S_abs = Σ |x[d-k]|·|x[d+k]|; for the complex P
   |dP| <= sqrt(2)·(2·h·nb + 2)·u·S_abs.  E (non-negative terms): one chain of 2 FMAs per term plus
   at most OPT + 2 = 10 adds of the shared-window split: |dE| <= (2·h·nb + 10)·u·E.  M = |P|²/E²
   as in model 1 (kM = 6).
4. fp64 overlap-save matched filter (zc_fftcorr.hip: mc_pers_kernel, mc_fused_kernel, and the rocFFT
   pipeline with mc_extract_kernel; u = 2^-53).  Block q with input span u_q (M samples, zero-padded as
   the kernel pads it) gives y = F*(F u_q ⊙ H / M), H = F h, h the reversed conjugated taps, L = log2(M).
   One transform has the normwise relative error eps = L·eta, eta = mu + gamma_4·(sqrt(2) + mu) as in
   model 2 (Higham Thm 24.2), with mu the absolute error of the worst twiddle as the code builds it.  A
   sincospi table entry is taken within 2 ulp per component (4u as a complex number), a complex product
   adds sqrt(2)·gamma_2 = 2.83u (Higham Lemma 3.5), a squaring doubles the error of its operand:
       mc_fused_kernel  mf_tw = product of two table entries 10.83u, squared 24.5u, squared again
                        51.8u, times the rounded constant of mf_rot8 (+2.83u)            mu = 55u
       mc_pers_kernel   tb / tc entry 4u, b^2 10.83u, b^4 24.5u, b^8 51.8u (the mf_w16 / mp_w32
                        constants multiply b and b^2 only)                               mu = 52u
       rocFFT           its tables are not part of this repository: taken no better than ours, mu = 55u
   Error of the block's output vector, first order, with ||a ⊙ b||_2 <= ||a||_2·||b||_inf:
       forward transform     eps_k·||F u||_2·||H||_inf / M            -> eps_k·kappa·||u_q||·||ref||
       H's own error         ||F u||_2·||dH||_inf / M, |dH_k| <= eps_r·||h||_1 (componentwise form of
                             the same theorem; H / M is exact, M a power of two) -> eps_r·lam·||u_q||·||ref||
       pointwise product     2.83u·||F u ⊙ H / M||_2                  -> 2.83u·kappa·||u_q||·||ref||
       inverse transform     eps_k·||y||_2                            -> eps_k·kappa·||u_q||·||ref||
   (each line after the inverse's factor sqrt(M)), kappa = ||F h||_inf / ||ref||_2 and lam = ||h||_1 /
   ||ref||_2 two properties of the taps (2.85 and 42.4 for the 2048 taps of tests/zc_mf_streams.py).  Every output of
   the block is bounded by the 2-norm of that vector:
       |d corr| <= K·u·L·||u_q||_2·||ref||_2,   K = (2·eta_k / u + 2.83 / L)·kappa + (eta_r / u)·lam.
   A worst-case bound: numpy's pocketfft measures 0.011 to 0.066 of u·L·||u_q||·||ref||, and the three
   GPU kernels 0.05 to 0.11: a few 1e-5 of it.
   The window energy is exact when the samples are integers (every prefix below 2^53); otherwise the
   prefix scan (|u|^2 with two roundings, at most 44 adds to any prefix in mc_pers_kernel, fewer in the
   others, one subtraction) gives |d e| <= ZC_OS_KE·u·E_block, "error relative to the block's energy".
   The counted roundings of each normaliser (ZC_NORM_K, in units of u, operations correctly rounded
   except the device sqrt and hypot, taken within 1 ulp = 2u) are listed at zc_norm_k().
"""
from __future__ import annotations

import math

import numpy as np

U32 = 2.0 ** -24
ETA = (1.0 + 4.0 * math.sqrt(2.0)) * U32          # per radix-2 stage (complex butterfly + twiddle)


def win_fast_k(E: int, NB: int = 1):
    """(kP, kR, kM) of model 1 for a window kernel with E samples per lane and NB branches."""
    return math.sqrt(2.0) * (E + 8 + NB), float(E + 11 + NB), 6.0


def zc_win_eps(N: int) -> float:
    """Model 2, fused window-FFT kernel: fp32 column FFTs of N/64 points (+2 stages)."""
    return (math.log2(max(N // 64, 2)) + 2) * ETA


def rocfft_eps(N: int) -> float:
    """Model 2, rocFFT leg: all log2(N) stages in fp32 (+2)."""
    return (math.log2(N) + 2) * ETA


def park_bounds(x: np.ndarray, N: int):
    """Model 3 for one stream x[nb, T] (complex128): per-output (bP, bE, S_abs, E) of Park fp32."""
    x = np.atleast_2d(x)
    nb, T = x.shape
    h = N // 2
    ds = np.arange(h, T - h)
    s = np.zeros(ds.size)
    e = np.zeros(ds.size)
    for br in range(nb):
        ax = np.abs(x[br])
        for k in range(h):
            s += ax[ds - k] * ax[ds + k]
        e += np.convolve(ax ** 2, np.ones(h))[ds + h - 1]       # Σ_{k<h} |x[d+k]|²
    return math.sqrt(2.0) * (2 * h * nb + 2) * U32 * s, (2 * h * nb + 10) * U32 * e


def metric_bound(c, R, M, bP, bR, kM: float = 6.0):
    """First-order bound of M = c²/R² given |dc| <= bP, |dR| <= bR (models 1 and 3)."""
    Rm = np.maximum(R, 1e-12)
    p = bP / Rm
    return 2.0 * (c / Rm) * p + p * p + 2.0 * M * (bR / Rm) + kM * U32 * M + 1e-300


def _win_abs(ax, lag, W, nout):
    """Σ_{k<W} ax[d+k]·ax[d+k+lag] for d < nout (fp64 prefix sums of non-negative terms)."""
    p = np.concatenate(([0.0], np.cumsum(ax[:-lag] * ax[lag:])))
    d = np.arange(nout)
    return p[d + W] - p[d]


def window_model(kind: str, x: np.ndarray, N: int, P, R, M, E: int = 4):
    """Model 1 for one stream x[nb, T] (complex128) and the oracle's P, R, M of `kind`
    ("sc", "comb", "minn"): per-output bounds (bM, bP, bR).  E = 4 is the widest lane
    (win_fast.hip pick(): E in {2, 4}), so the bound covers every instantiation."""
    x = np.atleast_2d(x)
    nb, T = x.shape
    nout = T - N + 1
    kP, kR, kM = win_fast_k(E, nb)
    S = np.zeros(nout)
    for br in range(nb):
        ax = np.abs(x[br])
        if kind in ("sc", "comb"):
            S += _win_abs(ax, N // 2, N // 2, nout)
        else:
            Q = N // 4
            s = _win_abs(ax, Q, Q, T - Q + 1 - Q)               # windows starting at any d' <= T-2Q
            S += s[:nout] + s[2 * Q:2 * Q + nout]
    P, R, M = np.asarray(P), np.asarray(R), np.asarray(M)
    bP = kP * U32 * S + U32 * np.abs(P)
    bR = kR * U32 * R
    c = np.maximum(P.real, 0.0) if kind == "minn" else np.abs(P)
    return metric_bound(c, R, M, bP, bR, kM), bP, bR


# ---------------------------------------------------------------- model 4 (fp64 overlap-save) -----
U64 = 2.0 ** -53
ZC_OS_MU = {"pers": 52.0, "fused": 55.0, "rocfft": 55.0, "numpy": 1.0}    # worst twiddle error / u
ZC_OS_KE = 96.0                     # |d e| <= ZC_OS_KE·u·E_block: 2·(2 + 44) + 1, rounded up
# mp_rsqrt (v_rsq_f64 seed + two Newton steps): relative error in units of u.  The public CDNA ISA guide
# states the seed's precision as 2^29 ulp (2^-23 relative); rsqrt_newton_worst() emulates the two steps
# from seeds that far off and measures 1.22u (tests/test_zc_mf_streams_host.py holds it below this).
ZC_RSQRT_U = 2.0


def zc_os_eta(kernel: str) -> float:
    """Model 4: eta of one radix-2 stage of `kernel`'s block transform."""
    mu = ZC_OS_MU[kernel] * U64
    return mu + 4.0 * U64 / (1.0 - 4.0 * U64) * (math.sqrt(2.0) + mu)


def zc_os_K(ref: np.ndarray, M: int, kernel: str) -> float:
    """Model 4: K of |d corr| <= K·u·log2(M)·||u_q||·||ref|| for these taps."""
    ref = np.asarray(ref, np.complex128)
    nr = float(np.sqrt(np.sum(np.abs(ref) ** 2)))
    h = np.zeros(M, np.complex128)
    h[:ref.size] = np.conj(ref[::-1])
    kappa = float(np.max(np.abs(np.fft.fft(h)))) * (1.0 + 1e-12) / nr
    lam = float(np.sum(np.abs(ref))) / nr
    L = math.log2(M)
    return (2.0 * zc_os_eta(kernel) / U64 + 2.0 * math.sqrt(2.0) / L) * kappa + zc_os_eta("rocfft") / U64 * lam


def zc_os_block_bound(unorm, ref: np.ndarray, M: int, kernel: str):
    """Model 4: the bound of every output of a block whose input span has the 2-norm `unorm` (array)."""
    nr = np.sqrt(np.sum(np.abs(np.asarray(ref, np.complex128)) ** 2))
    return zc_os_K(ref, M, kernel) * U64 * math.log2(M) * unorm * nr


def zc_norm_k(kernel: str, mode: str, nb: int):
    """Model 4, counted roundings in units of u: (k, kmag).  k bounds a component of a normalised
    output relative to the sum of its branch terms, kmag the magnitude's own operation.
      "div"   zc_mf_kernel and mc_extract_kernel: host sqrt(ref_energy) 1, device sqrt 2, product 1,
              division 1 = 5 per term, nb - 1 branch adds; COMBINED: e + 1e-12 adds 1 before the sqrt
              (halved by it) -> 6; magnitude: hypot 2.
      "pers"  mc_pers_kernel with the extract fused (one branch): rn_inv = 1 / host sqrt 2, mp_rsqrt
              ZC_RSQRT_U, their product 1, c·inv 1 = 4 + ZC_RSQRT_U (COMBINED + 1); magnitude mp_cabs:
              fma and product 2 halved by the root, mp_rsqrt ZC_RSQRT_U, x·rsqrt 1 = 2 + ZC_RSQRT_U.
      "fused" mc_fused_kernel with the extract fused: host sqrt 1, sqrt 2, product 1, reciprocal 1,
              c·inv 1 = 6 (COMBINED 7); magnitude sqrt(fma): 1 + 2 = 3.
    RAW / SUM: the branch adds only (0 for one branch); the direct kernel's are exact on integers."""
    adds = nb - 1
    if mode in ("raw", "sum"):
        k = 0.0 if mode == "raw" else float(adds)
    elif kernel == "pers":
        k = 4.0 + ZC_RSQRT_U + (1.0 if mode == "combined" else 0.0)
    elif kernel == "fused":
        k = 7.0 if mode == "combined" else 6.0
    else:
        k = (6.0 if mode == "combined" else 5.0) + adds
    kmag = {"pers": 2.0 + ZC_RSQRT_U, "fused": 3.0}.get(kernel, 2.0)
    return k, kmag


def rsqrt_newton_worst(n: int = 20000, seed_err: float = 2.0 ** -23) -> float:
    """Largest relative error, in units of u, of mp_rsqrt's two Newton steps y += (y/2)·(1 - (x·y)·y)
    (fp64 with fma, emulated here in float64 with a longdouble fma) over n values of x in [1, 4) from
    seeds y0 = x^-1/2·(1 ± seed_err)."""
    LD = np.longdouble
    rng = np.random.default_rng(7)
    x = np.concatenate([1.0 + 3.0 * rng.random(n), [1.0, 2.0, 4.0 - 2.0 ** -51, 1.0 + 2.0 ** -52]])
    worst = 0.0
    for sg in (1.0, -1.0, 0.5, -0.5):
        y = (1.0 / np.sqrt(x.astype(LD)) * LD(1.0 + sg * seed_err)).astype(np.float64)
        for _ in range(2):
            h = x * y
            r = (LD(1.0) - h.astype(LD) * y.astype(LD)).astype(np.float64)        # fma(-h, y, 1): one rounding
            y = (y.astype(LD) + (0.5 * y).astype(LD) * r.astype(LD)).astype(np.float64)   # fma(y/2, r, y)
        t = 1.0 / np.sqrt(x.astype(LD))
        worst = max(worst, float(np.max(np.abs(y.astype(LD) - t) / t)) / U64)
    return worst
