"""GPU: the receiver back-end (csrc/backend.hip) pinned on exact delay, tie and edge-cut frames.

Every case goes through core.receiver_backend_batched, one frame per delay, pilot pattern or edge position in a
single call of at most 256 frames, as complex128, complex64 and int16 (the frames are integer-valued: the three
formats carry the same numbers and only the widening load differs, so their outputs are compared word for
word).  A shape the register-staged rx_backend_fast_kernel takes runs twice: as dispatched ("fast") and under
variant BE_FAST = 0 ("generic", rx_backend_kernel); every other shape runs the generic kernel alone.

The reference is tests/backend_frames.py's model (the oracle's chain with the stream-edge rules written out;
test_backend_frames_host.py shows it is the oracle on interior frames and within 2e-11 / 1e-12 / 8e-10 of the
closed forms of sto / evm / gain).  Tolerances: those of test_gpu_parity.py::
test_receiver_backend_batched_vs_oracle for cfo, h, xa, evm and slope; sto = slope's times N / 2 pi; gain 1e-8
relative to max(1, |gain|); evm_db 1e-7.  A missed 2 pi wrap moves sto by more than 1e-2.

Which code each family reaches:
  delay  the unwrap's runs of ceil(U / 256) bins per thread, their stitching across threads and waves
         (unwrap_slope_1b with be_wave_totals; unwrap_slope), idle trailing threads, a 2 pi wrap on every run
         and wave boundary as d sweeps the odd delays; bin sets with k = 0, descending, beyond ±N/2, and under
         the fast kernel's mid-buffer reduction slots (slots_clear == false: block_sums<4, true>); fft_lds's lone
         radix-2 stage (n_fft 2, 8) and its absence (4); cp_len 0; n_used = n_fft.
  tie    np.unwrap's boundary rule (dm == -pi && dd > 0) on steps of exactly ±pi.
  edge   BeWindow::issue's guarded arm, BeCp::issue's !full arm, the zero-fill of load_window and
         place_window_fft, the CP correlation's per-pair guard in both kernels, T < n_fft, frames wholly outside
         the stream.  Each cut frame is also decoded inside the zero-padded stream at origin -P: negative origins
         reach be_origin unchecked (ofs_rx_backend_at takes any int64), and enter the tone's phase index alone.

Bin sets: centred (core.centered_subcarrier_indices, even n_used only: for an odd width it returns one bin
fewer), contiguous with k = 0, the same descending, "high" (up to N/2 + 31) and "low" (from -N/2 - 31).

The worst deviation per family, kernel and output is kept in MARGINS (tools/backend_margins.py prints the table
of profiles/backend_exact_margins.md from it).

With a single used bin (n_used = 1) the complex gain aligns the bin exactly: evm is then the gain denominator's
1e-12 (1.00009e-12 after rounding, evm_db -233.98) in the model and in both kernels alike (equal to the last bit
on every delay), while the closed form says evm = 0, evm_db = -240: for n_used = 1 evm_db is compared with the
model's like every output, and left out of the closed-form comparison, which the oracle itself does not meet.
"""
import functools

import numpy as np
import pytest
import torch

import backend_frames as F

pytestmark = pytest.mark.gpu

FORMATS = ("c128", "c64", "int16")
MARGINS = {}                                   # (family, kernel, output) -> [worst deviation, its tolerance]


def to_device(x, fmt):
    if fmt == "int16":
        return torch.from_numpy(np.stack([x.real, x.imag], -1).astype(np.int16)).cuda()
    return torch.from_numpy(x.astype(np.complex64 if fmt == "c64" else np.complex128)).cuda()


def run(x, ps, ds, pil, dat, N, cp, k, fmt, cfo=None, origin=None):
    from ofdm_sync_amd import core
    assert x.shape[0] <= 256
    out = core.receiver_backend_batched(to_device(x, fmt), ps, ds, pil, dat, n_fft=N, cp_len=cp, fs_hz=F.FS, bins=k,
                                        cfo_hz=cfo, origin=origin)
    return {key: out[key].cpu().numpy() for key in F.KEYS}


def kernels(variant, N, U, nb, cp):
    """The kernels a shape runs on: [(name, select)] with select() to call before the launch."""
    if not F.is_fast(N, U, nb, cp):
        return [("generic", lambda: variant("BE_FAST", None))]
    return [("fast", lambda: variant("BE_FAST", None)), ("generic", lambda: variant("BE_FAST", 0))]


def words(v):
    return np.ascontiguousarray(v).view(np.uint64)


def same_words(a, b, what, zero_cfo_signs=False):
    for key in F.KEYS:
        if key == "cfo" and zero_cfo_signs:
            assert np.array_equal(words(a[key] + 0.0), words(b[key] + 0.0)), (what, key)
        else:
            assert np.array_equal(words(a[key]), words(b[key])), (what, key)


def check(o, r, N, family, kernel, what, keys=F.KEYS):
    """o within the tolerances of r, frame by frame; the worst deviations go to MARGINS."""
    dev, tol = F.batch_deviations(o, r), F.batch_tolerances(r, N)
    for key in keys:
        i = int(np.argmax(dev[key] / tol[key]))
        m = MARGINS.setdefault((family, kernel, key), [0.0, 1.0])
        if dev[key][i] / tol[key][i] >= m[0] / m[1]:
            m[:] = [float(dev[key][i]), float(tol[key][i])]
        print(f"{family} {kernel} {what} {key}: worst {dev[key][i]:.3g} (tolerance {tol[key][i]:.3g}, frame {i})")
    for key in keys:
        bad = np.flatnonzero(~(dev[key] < tol[key]))
        assert bad.size == 0, (family, kernel, what, key, bad[:8], dev[key][bad[:8]], tol[key][bad[:8]])
    assert all(np.all(np.isfinite(o[key])) for key in F.KEYS), (family, kernel, what)


# ------------------------------------------------------------------------------------------
# delay frames
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def delay_reference(N, U, cp, name, count):
    """(delays, x for one branch, ps, ds, model outputs, closed forms).  The model of a one-branch frame is the
    model of the same frame on every branch: (A·t + A·t) / 2 and (A·t + A·t + A·t) / 3 are exact."""
    k = F.bin_sets(N, U)[name]
    d = F.odd_delays(N, k, count)
    x, ps, ds = F.delay_batch(N, cp, 1, d)
    r = F.stack([F.model(x[b], int(ps[b]), int(ds[b]), N, cp, F.FS, k, np.ones(U), F.data_ref(U), cfo=0.0)
                 for b in range(d.size)])
    return d, x, ps, ds, r, F.stack([F.delay_closed_form(N, k, di) for di in d])


@pytest.mark.parametrize("shape", F.DELAY_SHAPES, ids=str)
def test_delay_frames(shape, variant):
    N, U, cp, branches, count = shape
    sets = F.bin_sets(N, U)
    assert {"contiguous", "reversed"} <= set(sets) and (N != 1024 or U % 2 or cp != 72 or len(sets) == 5)
    for name, k in sets.items():
        d, x1, ps, ds, r, c = delay_reference(N, U, cp, name, count)
        for nb in branches:
            x = np.repeat(x1, nb, axis=1)
            for kern, select in kernels(variant, N, U, nb, cp):
                select()
                what = f"N{N} U{U} cp{cp} nb{nb} {name}"
                outs = [run(x, ps, ds, np.ones(U), F.data_ref(U), N, cp, k, fmt, cfo=np.zeros(d.size)) for fmt in FORMATS]
                for fmt, o in zip(FORMATS[1:], outs[1:]):
                    same_words(outs[0], o, (what, kern, fmt))
                o = outs[0]
                assert np.array_equal(words(o["cfo"]), words(np.zeros(d.size))), what      # the given cfo echoed
                check(o, r, N, "delay", kern, what)
                check(o, c, N, "delay_closed", kern, what, [key for key in F.KEYS if U > 1 or key != "evm_db"])
                # the unwrap and the fit alone: the model's on the kernel's own h
                fit = np.array([F.unwrap_fit(o["h"][b], k, N) for b in range(d.size)])
                ts = 1e-9 * np.maximum(1.0, np.abs(fit[:, 0]))
                assert np.all(np.abs(o["slope"] - fit[:, 0]) < ts), what
                assert np.all(np.abs(o["sto"] - fit[:, 1]) < ts * N / (2 * np.pi)), what
                if U >= 2:
                    assert np.all(np.abs(o["sto"] - d) < 1e-2), what


# ------------------------------------------------------------------------------------------
# tie frames
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F.TIE_SHAPES, ids=str)
def test_tie_frames(shape, variant):
    N, U, cp, nb = shape
    pil = F.tie_pilots(U)
    x, ps, ds = F.delay_batch(N, cp, nb, [0, 0, 0])
    for name, k in F.bin_sets(N, U).items():
        r = F.stack([F.model(x[b], int(ps[b]), int(ds[b]), N, cp, F.FS, k, pil[b], F.data_ref(U), cfo=0.0)
                     for b in range(3)])
        assert np.all(r["h"].imag == 0) and set(np.angle(r["h"]).ravel()) == {-np.pi, 0.0}
        for kern, select in kernels(variant, N, U, nb, cp):
            select()
            what = f"N{N} U{U} nb{nb} {name}"
            outs = [run(x, ps, ds, pil, F.data_ref(U), N, cp, k, fmt, cfo=np.zeros(3)) for fmt in FORMATS]
            for fmt, o in zip(FORMATS[1:], outs[1:]):
                same_words(outs[0], o, (what, kern, fmt))
            o = outs[0]
            # the preconditions, on the kernel's own h: exactly real, bit for bit the model's (the spectrum is
            # exactly (AMP, +0) and the LS division is numpy's on equal operands)
            assert np.all(o["h"].imag == 0), (what, kern)
            assert np.array_equal(words(o["h"]), words(r["h"])), (what, kern)
            check(o, r, N, "tie", kern, what)


# ------------------------------------------------------------------------------------------
# edge-cut frames
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_reference(N, U, cp, nb, name, short):
    k = F.bin_sets(N, U)[name]
    x, ps, ds, what, pil, dat, cfo = F.edge_batch(N, U, cp, nb, short)
    est = F.stack([F.model(x[b], int(ps[b]), int(ds[b]), N, cp, F.FS, k, pil[b], dat) for b in range(len(what))])
    giv = F.stack([F.model(x[b], int(ps[b]), int(ds[b]), N, cp, F.FS, k, pil[b], dat, cfo=float(cfo[b]))
                   for b in range(len(what))])
    return k, x, ps, ds, pil, dat, cfo, est, giv


@pytest.mark.parametrize("short", [False, True], ids=["long", "short"])
@pytest.mark.parametrize("shape", F.EDGE_SHAPES, ids=str)
def test_edge_cut_frames(shape, short, variant):
    N, U, cp, nb, name = shape
    k, x, ps, ds, pil, dat, cfo, est, giv = edge_reference(N, U, cp, nb, name, short)
    P = F.edge_pad(N, cp)
    xp = F.pad(x, P)
    org = np.full(ps.size, -P, np.int64)
    for kern, select in kernels(variant, N, U, nb, cp):
        select()
        for c, r in ((None, est), (cfo, giv)):
            what = f"N{N} U{U} cp{cp} nb{nb} {name} {'short' if short else 'long'} {'estimated' if c is None else 'given'} cfo"
            outs = [run(x, ps, ds, pil, dat, N, cp, k, fmt, cfo=c) for fmt in FORMATS]
            for fmt, o in zip(FORMATS[1:], outs[1:]):
                same_words(outs[0], o, (what, kern, fmt))
            check(outs[0], r, N, "edge", kern, what)
            if c is not None:
                assert np.array_equal(words(outs[0]["cfo"]), words(cfo)), what
            # the same kernel on the zero-padded stream, origin -P: word for word (a zero cfo of either sign)
            for fmt, o in zip(FORMATS, outs):
                padded = run(xp, ps + P, ds + P, pil, dat, N, cp, k, fmt, cfo=c, origin=org)
                same_words(o, padded, (what, kern, fmt, "padded"), zero_cfo_signs=c is None)


# ------------------------------------------------------------------------------------------
# the division both kernels and the helpers share
# ------------------------------------------------------------------------------------------
def test_division_has_numpys_signs_of_zero():
    """cdiv is documented as numpy's complex division bit for bit.  A zero numerator of either sign over
    denominators in every octant, and numerators that cancel exactly (a = 3 b): the signs of the zero parts are
    numpy's.  They decide the phase (0, -0, pi or -pi) of the channel estimate of a window outside the stream."""
    from ofdm_sync_amd import core
    rng = np.random.default_rng(11)
    n = 4096
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    z = np.empty(4, complex)
    z.real, z.imag = [0.0, 0.0, -0.0, -0.0], [0.0, -0.0, 0.0, -0.0]
    for a in (np.tile(z, n // 4), (b + 1e-9) * 3.0, (b + 1e-9) * (0.0 + 2.0j)):
        got = core.ls_channel_estimate(a[None], b[None])[0]
        assert np.array_equal(words(got), words(a / (b + 1e-9)))
