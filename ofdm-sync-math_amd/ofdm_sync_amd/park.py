"""Drop-in for ``park.park_streaming_metric`` (reference: park.py:64-114).

Like the reference, the symbol length is read from the module global ``N_FFT`` at call time.
Computed by ``ofs_park_metric`` (csrc/corr.hip): an LDS-staged direct mirror product, fp64
for complex128 / integer inputs, fp32 for complex64 tensors unless ``precision`` says otherwise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _chunked, _lib

N_FFT = 2048            # core.py:6


def _run(batch: _lib.Batch, N: int, prec: int):
    dev = batch.data.device
    half = N // 2
    nout = batch.T - 2 * half if (half > 0 and batch.T >= 2 * half + 1) else 0
    M = _lib.out_real((batch.B, nout), prec, dev)
    P = _lib.out_cplx((batch.B, nout), prec, dev)
    E = _lib.out_real((batch.B, nout), prec, dev)
    if nout > 0:
        rc = _lib.lib().ofs_park_metric(batch.fmt, batch.data.data_ptr(), batch.B, batch.nb, batch.T,
                                        int(N), prec, M.data_ptr(), P.data_ptr(), E.data_ptr(),
                                        _lib.stream_ptr())
        _lib.check(rc, "ofs_park_metric")
    ds = torch.arange(half, half + nout, dtype=torch.int64, device=dev)
    return ds, M, P, E


def park_streaming_metric(rx, *, precision=None):
    """Park timing metric across receive branches: returns (ds, M, P_sum, E_sum)."""
    batch = _lib.as_batch(rx, batched=False)
    prec = _lib.resolve_precision(batch, precision)
    ds, M, P, E = _run(batch, int(N_FFT), prec)
    if batch.from_numpy:
        return (_lib.to_host(ds), _lib.to_host(M[0], np.float64), _lib.to_host(P[0], np.complex128),
                _lib.to_host(E[0], np.float64))
    return ds, M[0], P[0], E[0]


def park_streaming_metric_batched(x, N: int | None = None, *, precision=None):
    """Batched Park metric over x[B, n_branch, T]: (ds, M, P, E), device tensors [B, T-2*(N//2)]."""
    batch = _lib.as_batch(x, batched=True)
    prec = _lib.resolve_precision(batch, precision)
    return _run(batch, int(N_FFT if N is None else N), prec)


# ---- resumable chunked form (csrc/park_chunk.hip, ofs_park_metric_chunk) -----------------------
# sample dtype -> (format, precision, real output dtype, complex output dtype)
_CHUNK_FORMATS = {
    torch.complex64: (_lib.C64, _lib.FP32, torch.float32, torch.complex64),
    torch.complex128: (_lib.C128, _lib.FP64, torch.float64, torch.complex128),
    torch.int16: (_lib.CI16, _lib.FP64, torch.float64, torch.complex128),
}


class ParkChunkResult:
    """Outputs of one ``ParkChunkedMetric.push``: ``M`` real, ``P`` complex, ``E`` real (float32 /
    complex64 for complex64 streams, float64 / complex128 otherwise), each ``[B, Tc]`` or None when not
    requested; ``d0`` ``[B]`` int64, the reference's centre index d of element 0 (element j belongs to
    d0 + j; elements with d < N // 2 are +0.0); ``peak_index`` ``[B]`` int64 and ``peak_value`` ``[B]``
    float64, the running argmax of M over the reference's outputs on the samples so far (its d and its
    M; -1 and 0.0 while there is none), or None without ``track_peak``."""
    __slots__ = ("M", "P", "E", "d0", "peak_index", "peak_value")

    def __init__(self, M, P, E, d0, peak_index, peak_value):
        self.M, self.P, self.E, self.d0 = M, P, E, d0
        self.peak_index, self.peak_value = peak_index, peak_value


class ParkChunkedMetric(_chunked.ChunkedStreams):
    """Resumable Park timing metric with a running peak over B streams that arrive in chunks
    (``ofs_park_metric_chunk``).

    The chunk-fed form of ``park_streaming_metric_batched``.  ``dtype`` fixes the sample format and the
    precision: ``torch.complex64`` (fp32), ``torch.complex128`` (fp64) or ``torch.int16`` (I/Q pairs in a
    trailing axis of 2, fp64).  ``push(x)`` takes the next ``Tc`` samples of every stream -
    ``[B, n_branch, Tc]`` (int16: ``[B, n_branch, Tc, 2]``), or without the branch axis for one branch -
    and returns M / P / E ``[B, Tc]`` at those samples: element j belongs to the stream's newest sample
    n = samples_seen + j, that is to the reference's centre index d = n - N // 2 + 1; ``d0`` holds the d
    of element 0 and elements with d < N // 2 are +0.0.  With ``track_peak`` every result also carries
    the running ``argmax(M)`` of each stream (the reference's detection, park.py:161-164), found on the
    device as the chunks pass; this needs M, so an M buffer is kept even when ``"M"`` is not in
    ``outputs`` (``M`` of the result is then None).  Interface and buffer ownership are those of
    ``_metrics.WindowMetricChunked``: ``push(x, final=True)`` or ``flush()`` leaves fresh streams, the
    result buffers are this object's (cached per ``Tc``, overwritten in stream order by a later ``push``
    of that length), ``push`` never synchronises.

    For any chunking of a stream of T >= 2 * (N // 2) + 1 samples, the concatenated outputs with their
    first 2 * (N // 2) - 1 elements dropped begin with, bit for bit, the one-shot batched call on the
    whole stream; one more element follows, d = T - N // 2, whose window ends at the last sample (the
    reference stops one output earlier: it asks for sample d + N // 2).  The peak follows the reference:
    an output joins it with the push that brings sample d + N // 2, so the last peak is
    ``ofs_row_argmax`` of the one-shot M.  Nothing is summed across calls, so the
    stream may be of any length.  ``N=None`` reads the module global ``N_FFT`` at construction; N,
    n_branch and dtype are fixed for the object's life.  N is at most 8190 (complex64) or 4094.
    """

    _entry, _sizes = "ofs_park_metric_chunk", "ofs_park_chunk"

    def __init__(self, B: int, n_branch: int = 1, N: int | None = None, dtype=torch.complex64,
                 outputs=("M", "P", "E"), track_peak: bool = True, device=None):
        if dtype not in _CHUNK_FORMATS:
            raise ValueError(f"dtype must be torch.complex64, torch.complex128 or torch.int16, got {dtype!r}")
        bad = [o for o in outputs if o not in ("M", "P", "E")]
        if bad:
            raise ValueError(f"outputs may name 'M', 'P' and 'E', got {bad}")
        N = int(N_FFT if N is None else N)
        self.fmt, self.precision, self._rdt, self._cdt = _CHUNK_FORMATS[dtype]
        super().__init__(B, device, (self.fmt, int(n_branch), N),
                         f"ParkChunkedMetric needs n_branch >= 1 and 2 <= N <= 8190 (complex64) or 4094 "
                         f"(complex128, int16) (got n_branch={n_branch}, N={N}, dtype={dtype}, B={B})")
        self.n_branch, self.N, self.dtype = int(n_branch), N, dtype
        self.outputs, self.track_peak = tuple(outputs), bool(track_peak)

    def _alloc(self, Tc: int):
        """(the result, the M buffer the call writes)."""
        B, dev, want = self.B, self.device, self.outputs
        M = torch.empty((B, Tc), dtype=self._rdt, device=dev) if "M" in want and Tc else None
        P = torch.empty((B, Tc), dtype=self._cdt, device=dev) if "P" in want and Tc else None
        E = torch.empty((B, Tc), dtype=self._rdt, device=dev) if "E" in want and Tc else None
        pi = torch.zeros((B,), dtype=torch.int64, device=dev) if self.track_peak else None
        pv = torch.zeros((B,), dtype=torch.float64, device=dev) if self.track_peak else None
        res = ParkChunkResult(M, P, E, torch.zeros((B,), dtype=torch.int64, device=dev), pi, pv)
        # the peak is folded from M: a private M buffer when the caller did not ask for M
        Mk = torch.empty((B, Tc), dtype=self._rdt, device=dev) if self.track_peak and M is None and Tc else M
        return res, Mk

    def _launch(self, x, Tc: int, final: int, bufs):
        r, Mk = bufs
        return self._fn(self.fmt, x, self.B, self.n_branch, Tc, self.N,
                        self.precision, self.state.data_ptr(), _lib.ptr(Mk), _lib.ptr(r.P), _lib.ptr(r.E),
                        r.d0.data_ptr(), _lib.ptr(r.peak_index), _lib.ptr(r.peak_value), final,
                        _lib.stream_ptr())

    def _call(self, x, Tc: int, final: bool) -> ParkChunkResult:
        return super()._call(x, Tc, final)[0]

    def _chunk(self, x, final: bool):
        return _chunked.complex_chunk(self, x, final, self.n_branch, self.dtype)
