"""Shared host wrappers for the sliding-window metrics (S&C / combined S&C / Minn)."""
from __future__ import annotations

import numpy as np
import torch

from . import _chunked, _lib

_SC, _COMB, _MINN = "sc", "comb", "minn"


def _empty(from_numpy: bool, dev):
    if from_numpy:
        return np.zeros(0), np.zeros(0, dtype=complex), np.zeros(0)
    return (torch.zeros(0, dtype=torch.float64, device=dev),
            torch.zeros(0, dtype=torch.complex128, device=dev),
            torch.zeros(0, dtype=torch.float64, device=dev))


def window_metric(kind: str, x, N: int, *, batched: bool, precision=None):
    """Run one of the S&C/Minn window metrics.  Returns (M, P, R).

    Unbatched: 1-D/2-D reference inputs -> numpy (or torch) arrays of length T-N+1.
    Batched: [B, n_branch, T] -> device tensors [B, T-N+1].
    """
    batch = _lib.as_batch(x, batched=batched)
    prec = _lib.resolve_precision(batch, precision)
    dev = batch.data.device
    N = int(N)
    n_out = batch.T - N + 1
    if kind in (_SC, _COMB):
        if N // 2 == 0 or n_out <= 0:
            if batched:
                return (_lib.out_real((batch.B, 0), prec, dev), _lib.out_cplx((batch.B, 0), prec, dev),
                        _lib.out_real((batch.B, 0), prec, dev))
            return _empty(batch.from_numpy, dev)
        if N % 2:
            # the reference slices x[0:half] against x[half:N] (N-half elements): broadcasting
            # fails for odd N (sc.py:60, combined_sc_min.py:150-151)
            raise ValueError(f"operands could not be broadcast together: odd symbol length {N}")
    else:
        if n_out <= 0:
            if batched:
                return (_lib.out_real((batch.B, 0), prec, dev), _lib.out_cplx((batch.B, 0), prec, dev),
                        _lib.out_real((batch.B, 0), prec, dev))
            return _empty(batch.from_numpy, dev)
    M = _lib.out_real((batch.B, n_out), prec, dev)
    P = _lib.out_cplx((batch.B, n_out), prec, dev)
    R = _lib.out_real((batch.B, n_out), prec, dev)
    L = _lib.lib()
    if kind == _MINN:
        rc = L.ofs_minn_metric(batch.fmt, batch.data.data_ptr(), batch.B, batch.nb, batch.T, N, prec,
                               M.data_ptr(), P.data_ptr(), R.data_ptr(), _lib.stream_ptr())
        _lib.check(rc, "ofs_minn_metric")
    else:
        rc = L.ofs_sc_metric(batch.fmt, batch.data.data_ptr(), batch.B, batch.nb, batch.T, N,
                             1 if kind == _COMB else 0, prec, M.data_ptr(), P.data_ptr(), R.data_ptr(),
                             _lib.stream_ptr())
        _lib.check(rc, "ofs_sc_metric")
    if batched:
        return M, P, R
    if batch.from_numpy:
        return (_lib.to_host(M[0], np.float64), _lib.to_host(P[0], np.complex128),
                _lib.to_host(R[0], np.float64))
    return M[0], P[0], R[0]


# ---- resumable chunked form (csrc/win_chunk.hip, ofs_win_metric_chunk) -------------------------
KINDS = {_SC: 1, _COMB: 2, _MINN: 3, 1: 1, 2: 2, 3: 3}        # ofs_win_plan kinds


class WindowChunkResult:
    """Outputs of one ``WindowMetricChunked.push``: ``M`` float32, ``P`` complex64, ``R`` float32, each
    ``[B, Tc]`` or None when not requested, and ``d0`` ``[B]`` int64, the reference's output index d of
    element 0 (element i belongs to d0 + i; negative while a stream fills, those elements are +0.0)."""
    __slots__ = ("M", "P", "R", "d0")

    def __init__(self, M, P, R, d0):
        self.M, self.P, self.R, self.d0 = M, P, R, d0


class WindowMetricChunked(_chunked.ChunkedStreams):
    """Resumable S&C / combined S&C / Minn timing metric over B complex64 streams that arrive in chunks
    (``ofs_win_metric_chunk``).

    The chunk-fed form of the streaming fp32 fast path behind ``window_metric``.  ``kind`` is "sc",
    "comb" or "minn" (or 1, 2, 3 as in ``ofs_win_plan``).  ``push(x)`` takes the next ``Tc`` samples of
    every stream - complex64 ``[B, n_branch, Tc]``, or ``[B, Tc]`` for one branch - and returns M / P / R
    ``[B, Tc]`` at those samples: element i belongs to the stream's newest sample n = samples_seen + i,
    that is to the reference's output index d = n - (symbol_len - 1); ``d0`` holds the d of element 0 and
    elements with d < 0 are +0.0.  Interface and buffer ownership are those of
    ``sync_aa.AAChunkedDetectorF32``: ``push(x, final=True)`` or ``flush()`` leaves fresh streams, the
    result buffers are this object's (cached per ``Tc``, overwritten in stream order by a later ``push``
    of that length), ``push`` enqueues one launch and never synchronises.

    For any chunking of a stream of T >= symbol_len samples, the concatenated outputs with their first
    symbol_len - 1 elements dropped equal, bit for bit, the one-shot batched call on the whole complex64
    stream (fp32, ``ofs_win_plan`` > 0) - whichever outputs are requested.  The state carries the fp64
    running row sums since sample 0: at unit amplitude their rounding reaches one fp32 ulp of a window
    sum after about ``2**30 * W`` samples (include/ofdmsync.h); a final call restarts them.
    The window W (symbol_len / 2, Minn: symbol_len / 4) is 128, 256, 512, 1024 or 2048 (2048: one
    branch); kind, n_branch and symbol_len are fixed for the object's life.
    """

    _entry, _sizes = "ofs_win_metric_chunk", "ofs_win_chunk"

    def __init__(self, kind, B: int, n_branch: int = 1, symbol_len: int = 2048,
                 outputs=("M", "P", "R"), device=None):
        if kind not in KINDS:
            raise ValueError(f"kind must be 'sc', 'comb' or 'minn' (or 1, 2, 3), got {kind!r}")
        self.kind = KINDS[kind]
        super().__init__(B, device, (self.kind, int(n_branch), int(symbol_len)),
                         f"WindowMetricChunked supports 1-2 branches and a window (symbol_len / 2, Minn: "
                         f"symbol_len / 4) of 128/256/512/1024/2048, 2048 with one branch "
                         f"(got kind={kind!r}, n_branch={n_branch}, symbol_len={symbol_len}, B={B})")
        bad = [o for o in outputs if o not in ("M", "P", "R")]
        if bad:
            raise ValueError(f"outputs may name 'M', 'P' and 'R', got {bad}")
        self.n_branch, self.symbol_len = int(n_branch), int(symbol_len)
        self.outputs = tuple(outputs)

    def _alloc(self, Tc: int) -> WindowChunkResult:
        B, dev, want = self.B, self.device, self.outputs
        M = torch.empty((B, Tc), dtype=torch.float32, device=dev) if "M" in want and Tc else None
        P = torch.empty((B, Tc), dtype=torch.complex64, device=dev) if "P" in want and Tc else None
        R = torch.empty((B, Tc), dtype=torch.float32, device=dev) if "R" in want and Tc else None
        return WindowChunkResult(M, P, R, torch.zeros((B,), dtype=torch.int64, device=dev))

    def _launch(self, x, Tc: int, final: int, r: WindowChunkResult):
        return self._fn(self.kind, x, self.B, self.n_branch, Tc, self.symbol_len,
                        self.state.data_ptr(), _lib.ptr(r.M), _lib.ptr(r.P), _lib.ptr(r.R), r.d0.data_ptr(),
                        final, _lib.stream_ptr())

    def _chunk(self, x, final: bool):
        return _chunked.complex_chunk(self, x, final, self.n_branch, torch.complex64, "complex64")


class SCMinnChunked:
    """Combined S&C (kind 2) and Minn (kind 3) on the same chunks, two launches per ``push``: returns
    ``(minn, sc)`` results, each as ``WindowMetricChunked`` returns them.  The yardsticks are the two
    separate one-shot calls (not the fused ``ofs_sc_minn_metric``, whose S&C energy rounds differently)."""

    def __init__(self, B: int, n_branch: int = 1, symbol_len: int = 2048, outputs=("M", "P", "R"), device=None):
        self.minn = WindowMetricChunked(_MINN, B, n_branch, symbol_len, outputs=outputs, device=device)
        self.sc = WindowMetricChunked(_COMB, B, n_branch, symbol_len, outputs=outputs, device=device)
        self.max_chunk = min(self.minn.max_chunk, self.sc.max_chunk)

    @property
    def samples_seen(self) -> int:
        return self.sc.samples_seen

    def push(self, x: torch.Tensor, final: bool = False):
        x, Tc = self.sc._chunk(x, final)
        return self.minn._call(x, Tc, final), self.sc._call(x, Tc, final)

    def flush(self):
        return self.minn.flush(), self.sc.flush()

    def reset(self, mask: torch.Tensor | None = None) -> None:
        self.minn.reset(mask)
        self.sc.reset(mask)
