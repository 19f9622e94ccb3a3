"""Exact frames for the receiver back-end (csrc/backend.hip: rx_backend_kernel and rx_backend_fast_kernel).

NumPy and the CPU oracle's conventions only; no GPU code.  model() restates ofdm_oracle.rx_backend with the rules
at the stream's edges written out - the oracle cannot express them, because a negative numpy slice start wraps
around.  Both kernels agree on these rules (load_window / place_window_fft, BeWindow::issue,
BeCp::issue and the generic kernel's CP loop):

  * zero-fill: a window sample whose stream index i lies outside [0, T) is +0.  The branch sum starts from
    +0, so a zero sample is (+0, +0) whatever the sign of the tone's components;
  * pair-drop: a CP pair (ps + n, ps + N + n), n < cp, counts only if both indices are in [0, T); with no pair
    left P = 0 and cfo = -angle(0)·fs/(2 pi N) = -0.0;
  * the tone's phase index of stream sample i is origin + i (origin 0 unless the frame was cut out of a stream);
    origin enters nothing else and may be negative;
  * a frame whose windows lie wholly outside the stream has a zero spectrum: h = ±0 (the sign of each part is
    the division's), xa = gain = 0, evm = 1; the phases are then 0 or ±pi and the slope is whatever np.unwrap
    and the fit make of them.

Frame families (every sample an integer, so complex64, complex128 and int16 carry the same numbers):

  delay  zero but for AMP at ps + cp + d and ds + cp + d, pilots 1, cfo = 0.0 given.  The pilot spectrum is
         AMP·exp(-2 pi i k d / N): sto = d, slope = -2 pi d / N (times skk / (skk + 1e-12), skk = sum kz^2, which
         is 0 for a single bin), and with ref[u] = 1, but 1j where u % 4 == 3, xhat = 1 on every bin, so
         xa = gain = mean(ref) and evm = sqrt(mean|mean(ref) - ref|^2 / mean|ref|^2), about 0.6.  With odd d no
         phase step is within 2 pi / N of ±pi; centred bins skip k = 0 (a double step), so d < N/4 there and
         d < N/2 for contiguous bins.
  tie    a delay frame with d = 0 and real pilots of mixed sign: any correct FFT gives exactly (AMP, +0) on every
         bin, h = AMP / (p + 1e-9) is exactly real (imaginary part +0 for p > 0, -0 for p < 0), every phase is 0
         or -pi and every step 0 or ±pi: np.unwrap's boundary rule (dm == -pi and dd > 0 -> +pi) leaves the
         phases as they are, a kernel without it loses 2 pi at each +pi step.
  edge   round(300·gaussian) frames whose CP, pilot window or data window is cut by the stream's start or end.
"""
import math

import numpy as np

FS = 1.0e6
AMP = 1000.0
BW = 256                                   # threads per frame in backend.hip
KEYS = ("cfo", "h", "xa", "gain", "evm", "evm_db", "slope", "sto")


# ------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------
def unwrap_fit(h, bins, n_fft):
    """(slope, sto) of estimate_timing_offset_from_phase_slope as ofdm_oracle.rx_backend states it."""
    k = np.asarray(bins)
    phi = np.unwrap(np.angle(h))
    kz = k.astype(float) - np.mean(k.astype(float))
    pz = phi - np.mean(phi)
    slope = float(np.sum(kz * pz) / (float(np.sum(kz * kz)) + 1e-12))
    return slope, float(-slope * n_fft / (2 * np.pi))


def model(x, ps, ds, n_fft, cp, fs, bins, pil, dat, cfo=None, origin=0):
    """ofdm_oracle.rx_backend, expression for expression, with the stream-edge rules of the header."""
    x = np.asarray(x)
    x = (x[np.newaxis, :] if x.ndim == 1 else x).astype(np.complex128, copy=False)
    T = x.shape[1]
    if cfo is None:
        n = np.arange(cp)
        ok = (ps + n >= 0) & (ps + n_fft + n < T)                       # pair-drop
        a = x[:, ps + n[ok]]
        b = x[:, ps + n_fft + n[ok]]
        P = np.sum(a * np.conj(b))
        cfo = float(-np.angle(P) * fs / (2 * np.pi * n_fft))
    k = np.asarray(bins)

    def used(s):
        i = s + cp + np.arange(n_fft)
        ok = (i >= 0) & (i < T)                                         # zero-fill
        n = (origin + i[ok]).astype(float)
        tone = np.exp(1j * 2 * np.pi * (-cfo) * n / fs)
        eff = np.zeros(n_fft, np.complex128)
        eff[ok] = np.mean(x[:, i[ok]] * tone[np.newaxis, :], axis=0)
        eff = eff + 0.0                                                 # a zero sample is (+0, +0)
        spec = np.fft.fftshift(np.fft.fft(eff, n=n_fft))
        return spec[(n_fft // 2 + k) % n_fft]

    h = used(ps) / (np.asarray(pil) + 1e-9)
    slope, sto = unwrap_fit(h, k, n_fft)
    xhat = used(ds) / (h + 1e-9)
    ref = np.asarray(dat)
    g = np.vdot(xhat, ref) / (np.vdot(xhat, xhat) + 1e-12)
    xa = xhat * g
    evm = float(np.sqrt(np.mean(np.abs(xa - ref) ** 2) / np.mean(np.abs(ref) ** 2)))
    return dict(cfo=float(cfo), h=h, xa=xa, gain=complex(g), evm=evm, evm_db=float(20 * np.log10(evm + 1e-12)),
                slope=slope, sto=sto)


def pad(x, P):
    """P zeros at each end of every branch."""
    x = np.asarray(x)
    return np.concatenate([np.zeros(x.shape[:-1] + (P,), x.dtype), x, np.zeros(x.shape[:-1] + (P,), x.dtype)], -1)


# ------------------------------------------------------------------------------------------
# tolerances: test_gpu_parity.py::test_receiver_backend_batched_vs_oracle's for cfo, h, xa, evm, slope;
# sto = slope's times N / 2 pi; gain as xa, of which it is a factor; evm_db the golden test's 1e-7
# ------------------------------------------------------------------------------------------
def tolerances(r, n_fft):
    """{output: absolute bound} for a frame whose reference outputs are r."""
    ts = 1e-9 * max(1.0, abs(r["slope"]))
    return dict(cfo=1e-6, h=1e-9 * max(1.0, float(np.max(np.abs(r["h"])))),
                xa=1e-8 * max(1.0, float(np.max(np.abs(r["xa"])))),
                gain=1e-8 * max(1.0, abs(r["gain"])), evm=1e-8 * max(1.0, r["evm"]), evm_db=1e-7,
                slope=ts, sto=ts * n_fft / (2 * np.pi))


def deviations(o, r):
    """{output: largest absolute difference} between two frames' outputs."""
    return {key: float(np.max(np.abs(np.asarray(o[key]) - np.asarray(r[key])))) for key in KEYS}


# ------------------------------------------------------------------------------------------
# bin sets
# ------------------------------------------------------------------------------------------
def centered(U):
    """core.centered_subcarrier_indices for an even U: -U/2 .. -1, 1 .. U/2."""
    assert U % 2 == 0
    return np.concatenate((np.arange(-(U // 2), 0), np.arange(1, U // 2 + 1)))


def bin_sets(N, U):
    """{name: bins} of the sets that exist for (N, U).  high: the upper end at N/2 + 31, so k mod N lands in
    [N/2, N/2 + 64) - the fast kernel's mid-buffer reduction slots; low: the lower end at -N/2 - 31."""
    sets = {}
    if U % 2 == 0:
        sets["centered"] = centered(U)
    c = np.arange(U) - U // 2
    sets["contiguous"] = c
    sets["reversed"] = c[::-1].copy()
    if U + 64 <= N:
        sets["high"] = np.arange(U) + (N // 2 + 31 - (U - 1))
        sets["low"] = np.arange(U) - (N // 2 + 31)
    return sets


def odd_delays(N, bins, count=None):
    """The odd d for which np.unwrap cannot alias: below N/4 when the set has a double step (centred), below
    N/2 otherwise; `count` of them spread over the range, the largest included."""
    k = np.asarray(bins)
    step = int(np.max(np.abs(np.diff(k)))) if k.size > 1 else 1
    d = np.arange(1, N // (2 * step), 2)
    if d.size == 0:                                  # N = 2, or N = 4 centred: d = 1 would put a step on ±pi
        return np.zeros(1, np.int64)
    if count is not None and d.size > count:
        d = d[np.round(np.linspace(0, d.size - 1, count)).astype(int)]
    return d


# ------------------------------------------------------------------------------------------
# delay and tie frames
# ------------------------------------------------------------------------------------------
def data_ref(U):
    """1, but 1j where u % 4 == 3; for U = 2 and 3 (no such u) the last bin is 1j, so that evm stays of order
    0.5.  A single bin always aligns exactly: there evm = 1e-12 / (|xhat|^2 + 1e-12) whatever the reference."""
    ref = np.ones(U, np.complex128)
    ref[np.arange(U) % 4 == 3] = 1j
    if 2 <= U < 4:
        ref[-1] = 1j
    return ref


def delay_batch(N, cp, nb, delays):
    """(x [B, nb, T], ps, ds) with one frame per delay, ps = 3, ds = ps + N + cp, 5 spare samples behind."""
    delays = np.asarray(delays)
    B = delays.size
    ps = np.full(B, 3, np.int64)
    ds = ps + N + cp
    x = np.zeros((B, nb, 2 * (N + cp) + 8), np.complex128)
    for b, d in enumerate(delays):
        x[b, :, ps[b] + cp + d] = AMP
        x[b, :, ds[b] + cp + d] = AMP
    return x, ps, ds


def delay_closed_form(N, bins, d):
    """The eight outputs of a delay frame (pilots 1, ref = data_ref) in closed form."""
    k = np.asarray(bins).astype(np.int64)
    ref = data_ref(k.size)
    h = AMP * np.exp(-2j * np.pi * ((k * int(d)) % N) / N) / (1 + 1e-9)
    kz = k - np.mean(k)
    skk = float(np.sum(kz * kz))
    slope = -2 * np.pi * d / N * skk / (skk + 1e-12)
    m = np.mean(ref)
    evm = float(np.sqrt(np.mean(np.abs(m - ref) ** 2) / np.mean(np.abs(ref) ** 2)))
    return dict(cfo=0.0, h=h, xa=np.full(k.size, m), gain=complex(m), evm=evm,
                evm_db=float(20 * np.log10(evm + 1e-12)), slope=float(slope), sto=float(-slope * N / (2 * np.pi)))


TIE_PATTERNS = ("+-+-", "++--", "----")


def tie_pilots(U):
    """[3, U] real pilots: + - + -, + + - - and all -."""
    return np.array([[1.0 if pat[u % 4] == "+" else -1.0 for u in range(U)] for pat in TIE_PATTERNS]).astype(complex)


# ------------------------------------------------------------------------------------------
# edge-cut frames
# ------------------------------------------------------------------------------------------
def integer_frames(B, nb, T, seed):
    """round(300·gaussian), as test_gpu_parity's back-end frames: exact in complex64, complex128 and int16."""
    rng = np.random.default_rng(seed)
    return np.round((rng.standard_normal((B, nb, T)) + 1j * rng.standard_normal((B, nb, T))) * 300)


def unit_symbols(shape, seed):
    return np.exp(2j * np.pi * np.random.default_rng(seed).random(shape))


def edge_positions(N, cp, T):
    """[(pilot_start, data_start, what)] for a stream of T >= 2 (N + cp) + 8 samples.  pilot_start runs from
    -(cp + N + 3) to +3 (every value where that is at most 150 frames, else ±3 around each place where the cut
    changes kind: 0, -cp, -(cp + N), a thread's stride of BW samples into the window, the window's middle), the
    data window then ends 1, cp and N - 1 samples past T, both windows leave the stream, and the CP keeps a
    single pair at either end."""
    lo = -(cp + N + 3)
    if 4 - lo <= 150:
        head = list(range(lo, 4))
    else:
        marks = (0, -cp, -(cp + N), -(cp + BW), -(cp + N // 2), -(cp + N - 1))
        head = sorted({m + e for m in marks for e in range(-3, 4) if lo <= m + e <= 3})
    pos = [(p, p + N + cp, "head") for p in head]
    for e in sorted({1, max(cp, 2), N - 1}):
        pos.append((5, T + e - cp - N, "tail"))                        # the data window ends e past T
    pos.append((T - (N + cp) - 2, T - 2, "tail"))                       # the data CP starts 2 before the end
    pos.append((-(cp + N) - 10, T + 5, "outside"))                      # nothing of either window is inside
    pos.append((-(cp + N), 7, "outside"))                               # pilot window outside, data inside
    pos.append((7, T - cp, "outside"))                                  # data window outside, pilot inside
    if cp >= 1:
        pos.append((-(cp - 1), N + 9, "one_pair"))                      # the pair n = cp - 1 alone: i0 = 0
        pos.append((T - 1 - N, 3, "one_pair"))                          # the pair n = 0 alone: i1 = T - 1
    return pos


def short_positions(N, cp, T):
    """Positions for a stream shorter than one window (T < n_fft)."""
    assert T < N
    return [(-cp, -cp - 2, "short"), (-cp - 1, T - cp - 1, "short"), (-cp - (N - T), 0, "short"), (0, -cp, "short"),
            (-cp - N + 1, T - cp - 1, "short")]


def closed_evm(U):
    ref = data_ref(U)
    return math.sqrt(float(np.mean(np.abs(np.mean(ref) - ref) ** 2) / np.mean(np.abs(ref) ** 2)))


# ------------------------------------------------------------------------------------------
# the shapes of tests/test_gpu_backend_exact.py (test_backend_frames_host.py checks the model on the same)
# ------------------------------------------------------------------------------------------
def is_fast(N, U, nb, cp):
    """ofs_rx_backend's dispatch: the register-staged kernel's shapes."""
    return nb in (1, 2) and cp <= 2 * BW and (N, U <= {1024: 768, 2048: 1280, 4096: 2560}.get(N, 0)) in \
        ((1024, True), (2048, True), (4096, True))


# (n_fft, n_used, cp_len, branches, delays per bin set or None for every odd d)
DELAY_SHAPES = [(1024, U, 72, (1, 2), None) for U in (1, 2, 63, 255, 256, 257, 768)] + [
    (2048, 1280, 144, (1, 2), 64), (4096, 2560, 288, (1, 2), 64),
    (1024, 256, 0, (1,), None),                      # cp_len = 0 (both kernels)
    (1024, 257, 512, (2,), None),                    # cp_len 512: the fast kernel's largest
    (1024, 257, 513, (2,), None),                    # ... and one more: the generic kernel
    (2, 2, 1, (1,), None), (4, 4, 1, (1,), None), (8, 8, 2, (1,), None),     # n_used = n_fft, lone radix-2 stage or not
    (64, 40, 16, (2,), None), (256, 100, 64, (3,), None),
    (1024, 769, 72, (2,), None),                     # one bin above the fast limit
    (1024, 256, 72, (3,), None),                     # three branches: the generic kernel
    (64, 40, 0, (1,), None)]                         # cp_len = 0, generic
TIE_SHAPES = [(1024, 257, 72, 1), (1024, 768, 72, 2), (256, 100, 64, 3)]          # (n_fft, n_used, cp_len, branches)
# (n_fft, n_used, cp_len, branches, bin set)
EDGE_SHAPES = [(1024, 256, 72, 2, "centered"), (1024, 257, 512, 1, "high"), (1024, 257, 513, 1, "high"),
               (1024, 768, 72, 2, "contiguous"), (1024, 769, 72, 2, "contiguous"), (1024, 256, 72, 3, "centered"),
               (1024, 63, 0, 1, "reversed"), (2048, 1280, 144, 1, "centered"), (4096, 2560, 288, 2, "low"),
               (2, 2, 1, 1, "contiguous"), (4, 4, 1, 1, "centered"), (8, 8, 2, 1, "contiguous"),
               (64, 40, 16, 2, "centered"), (64, 40, 0, 1, "contiguous"), (256, 100, 64, 3, "low")]


def edge_batch(N, U, cp, nb, short=False):
    """(x [B, nb, T], ps, ds, what, pil [B, U], dat [U], cfo [B]) of one edge-cut call: every position of
    edge_positions on a stream of 2 (N + cp) + 8 samples, or of short_positions on one of N - max(N/4, 1)."""
    T = N - max(N // 4, 1) if short else 2 * (N + cp) + 8
    pos = short_positions(N, cp, T) if short else edge_positions(N, cp, T)
    B = len(pos)
    seed = N * 7 + U + cp + nb + (1 if short else 0)
    x = integer_frames(B, nb, T, seed)
    ps = np.array([p[0] for p in pos], np.int64)
    ds = np.array([p[1] for p in pos], np.int64)
    cfo = np.random.default_rng(seed + 1).uniform(-4000.0, 4000.0, B)
    return x, ps, ds, [p[2] for p in pos], unit_symbols((B, U), seed + 2), unit_symbols(U, seed + 3), cfo


def edge_pad(N, cp):
    """Zeros enough at each end to bring every window of edge_positions / short_positions inside."""
    return N + cp + 16


def stack(frames):
    """[{output: value}] of a batch -> {output: array with the batch in front}."""
    return {key: np.array([f[key] for f in frames]) for key in KEYS}


def batch_tolerances(r, n_fft):
    """tolerances() for a stacked batch: {output: [B] absolute bounds}."""
    ts = 1e-9 * np.maximum(1.0, np.abs(r["slope"]))
    B = ts.size
    return dict(cfo=np.full(B, 1e-6), h=1e-9 * np.maximum(1.0, np.max(np.abs(r["h"]), axis=1)),
                xa=1e-8 * np.maximum(1.0, np.max(np.abs(r["xa"]), axis=1)),
                gain=1e-8 * np.maximum(1.0, np.abs(r["gain"])), evm=1e-8 * np.maximum(1.0, r["evm"]),
                evm_db=np.full(B, 1e-7), slope=ts, sto=ts * n_fft / (2 * np.pi))


def batch_deviations(o, r):
    """{output: [B] largest absolute difference per frame}."""
    out = {}
    for key in KEYS:
        d = np.abs(np.asarray(o[key]) - np.asarray(r[key]))
        out[key] = d.reshape(d.shape[0], -1).max(axis=1)
    return out
