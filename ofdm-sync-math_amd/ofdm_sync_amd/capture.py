"""Frame capture for chunk-fed streams (``ofs_frame_capture_chunk``, csrc/frame_capture.hip).

The chunked detectors report an event after the frame's samples have left; ``FrameCapture`` keeps a
ring of raw samples per stream on the device, takes trigger indices straight from a detector's event
buffers and emits each frame ``[start, start + frame_len)`` once its last sample has arrived.  The
frames go to ``core.receiver_backend_batched(..., origin=start)``::

    det = sync_aa.AAChunkedDetectorF32(B, n_ant, L, outputs=())
    cap = FrameCapture(B, n_ant, frame_len=F, history=H)
    for chunk in chunks:
        ev = det.push(chunk)
        res = cap.push(chunk, ev.ev_int[:, :, 3], ev.n_events)      # no host round trip
        b, slot, frames, start = cap.live(res)                       # the one synchronisation
        if len(b):
            out = core.receiver_backend_batched(frames, pilot_start - start, data_start - start, ...,
                                                origin=start)

Without the synchronisation: ``FrameCapture(..., compact_rows=R).push_compact`` writes the frames densely
with their number in device memory (``ofs_frame_capture_compact``), the back-end takes that number from
there (``n_active``), and ``StreamReceiver`` ties the two together::

    cap = FrameCapture(B, n_ant, frame_len=F, history=H, compact_rows=2 * B)
    rx = StreamReceiver(cap, pilot_offset, data_offset, pilot_used, data_used, n_fft=N, cp_len=cp, fs_hz=fs)
    for chunk in chunks:
        ev = det.push(chunk)
        res, dec = rx.push(chunk, ev.ev_int[:, :, 3], ev.n_events)  # enqueued; nothing read on the host
        # rows [0, res.n_rows[0]) of res.frames / res.frame_start / res.frame_stream and of dec are valid
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _chunked, _lib, core

_FORMATS = {torch.complex64: _lib.C64, torch.complex128: _lib.C128, torch.int16: _lib.CI16}
MAX_PENDING = 16
SCAN_BLOCK = 4096             # streams per block of the compact form's count-and-scan workgroup (FC_SCAN_BLK)


@dataclass
class FrameCaptureResult:
    """Outputs of one ``FrameCapture.push`` (the capture's own device buffers, overwritten in stream
    order by the next push): ``frames`` ``[B, Q, n_br, F]`` (int16: a trailing I/Q axis of 2),
    ``frame_start`` ``[B, Q]`` int64 (-1 for a slot the call did not write), ``n_frames`` ``[B]`` int32,
    ``dropped`` ``[B, 3]`` int32 = this call's triggers that came late / found the queue full / were
    cut by the stream's end.  The sample words of unwritten slots keep what they held."""
    frames: torch.Tensor
    frame_start: torch.Tensor
    n_frames: torch.Tensor
    dropped: torch.Tensor


@dataclass
class CompactFrames:
    """Outputs of one ``FrameCapture.push_compact`` (the capture's own device buffers, overwritten in
    stream order by the next ``push_compact``): ``frames`` ``[cap, n_br, F]`` (int16: a trailing I/Q axis
    of 2), ``frame_start`` ``[cap]`` int64 and ``frame_stream`` ``[cap]`` int32 (-1 from row ``n_rows[0]``
    on), ``row0`` ``[B]`` int32 (the first row of each stream's frames: the exclusive prefix sum of
    ``n_frames``), ``n_rows`` ``[2]`` int32 = rows written, frames lost because ``cap`` rows were taken,
    ``n_frames`` ``[B]`` and ``dropped`` ``[B, 3]`` as in ``FrameCaptureResult``.  Rows are in (stream,
    slot) order, the order ``FrameCapture.live`` returns."""
    frames: torch.Tensor
    frame_start: torch.Tensor
    frame_stream: torch.Tensor
    row0: torch.Tensor
    n_rows: torch.Tensor
    n_frames: torch.Tensor
    dropped: torch.Tensor


class FrameCapture(_chunked.ChunkedStreams):
    """Resumable frame capture over B streams that arrive in chunks (``ofs_frame_capture_chunk``).

    ``push(x, starts, n_starts)`` takes the next ``Tc`` samples of every stream - ``[B, n_br, Tc]`` of
    ``dtype`` (int16: ``[B, n_br, Tc, 2]``), or without the branch axis for one branch - and this call's
    triggers: ``starts`` is an int64 device tensor ``[B, K]`` with ANY strides, read in place (so a
    detector's ``ev_int[:, :, 3]`` of the same push works as it is), ``n_starts`` ``[B]`` int32 says how
    many of each row count (None: all K).  ``offset`` is added to every trigger.  Per stream, with n0
    samples before the call: a trigger ``s < max(0, n0 - history)`` is late and dropped; with
    ``max_pending`` starts waiting it is dropped as well; otherwise it waits until sample
    ``s + frame_len - 1`` has arrived and the frame is written to the next slot of that call's result, in
    the input's own format, bit for bit, for any chunking.  ``push(x, final=True)`` / ``flush()`` count
    the starts still waiting as cut by the stream's end and leave fresh streams; ``reset(mask)`` forgets
    streams without counting.  The result buffers are this object's (one set, overwritten in stream
    order by the next push - clone what must outlive it); ``push`` never synchronises, ``live`` does.
    ``history`` (default ``frame_len``) is how many samples before the current chunk stay retrievable:
    size it from the detector's delay, e.g. the gate length plus the chunk length for an [A][A] event.

    ``compact_rows=R`` adds ``push_compact`` (``ofs_frame_capture_compact``): the same capture on the same
    state - a stream may alternate between the two calls - with the frames of a call written densely
    into ``R`` rows and their number left on the device (``CompactFrames``); a frame for which no row is
    left is lost and counted in ``n_rows[1]``.  ``push_compact`` never synchronises either.
    """

    _entry, _sizes = "ofs_frame_capture_chunk", "ofs_frame_capture"

    def __init__(self, B: int, n_br: int = 1, frame_len: int = 0, history: int | None = None,
                 max_pending: int = 2, offset: int = 0, dtype=torch.complex64, device=None,
                 compact_rows: int | None = None):
        if dtype not in _FORMATS:
            raise ValueError(f"dtype must be torch.complex64, torch.complex128 or torch.int16, got {dtype!r}")
        history = int(frame_len if history is None else history)
        self.fmt = _FORMATS[dtype]
        super().__init__(B, device, (self.fmt, int(n_br), int(frame_len), history, int(max_pending)),
                         f"FrameCapture needs n_br >= 1, frame_len >= 1, history >= frame_len and max_pending in "
                         f"1..{MAX_PENDING} (got n_br={n_br}, frame_len={frame_len}, history={history}, "
                         f"max_pending={max_pending}, B={B})")
        self.n_br, self.frame_len, self.history = int(n_br), int(frame_len), history
        self.max_pending, self.offset, self.dtype = int(max_pending), int(offset), dtype
        iq = (2,) if dtype == torch.int16 else ()
        dev, Q = self.device, self.max_pending
        self._res = FrameCaptureResult(
            torch.zeros((self.B, Q, self.n_br, self.frame_len, *iq), dtype=dtype, device=dev),
            torch.full((self.B, Q), -1, dtype=torch.int64, device=dev),
            torch.zeros((self.B,), dtype=torch.int32, device=dev),
            torch.zeros((self.B, 3), dtype=torch.int32, device=dev))
        self._all: dict = {}                                      # K -> n_starts of "all K"
        self.compact_rows = None if compact_rows is None else int(compact_rows)
        self._compact = None
        if self.compact_rows is not None:
            R = self.compact_rows
            if not 1 <= R <= 2**31 - 1:
                raise ValueError(f"compact_rows must be in 1 .. 2^31 - 1, got {compact_rows}")
            self._compact = CompactFrames(
                torch.zeros((R, self.n_br, self.frame_len, *iq), dtype=dtype, device=dev),
                torch.full((R,), -1, dtype=torch.int64, device=dev),
                torch.full((R,), -1, dtype=torch.int32, device=dev),
                torch.zeros((self.B,), dtype=torch.int32, device=dev),
                torch.zeros((2,), dtype=torch.int32, device=dev),
                torch.zeros((self.B,), dtype=torch.int32, device=dev),
                torch.zeros((self.B, 3), dtype=torch.int32, device=dev))
            self._fn_compact = _lib.lib().ofs_frame_capture_compact

    def _alloc(self, Tc: int) -> FrameCaptureResult:
        return self._res                                          # one result, whatever the chunk length

    def _chunk(self, x, final: bool):
        return _chunked.complex_chunk(self, x, final, self.n_br, self.dtype)

    def _head(self, x, Tc: int, starts, n_starts) -> tuple:
        """The arguments both entry points begin with, up to the state."""
        trig = (None, 0, 0, None, 0)
        if starts is not None:
            K = int(starts.shape[1])
            trig = (starts.data_ptr(), starts.stride(0), starts.stride(1), n_starts.data_ptr(), K)
        return (self.fmt, x, self.B, self.n_br, Tc, self.frame_len, self.history, self.max_pending, self.offset,
                *trig, self.state.data_ptr())

    def _launch(self, x, Tc: int, final: int, r: FrameCaptureResult, starts=None, n_starts=None):
        return self._fn(*self._head(x, Tc, starts, n_starts), r.frames.data_ptr(), r.frame_start.data_ptr(),
                        r.n_frames.data_ptr(), r.dropped.data_ptr(), final, _lib.stream_ptr())

    def _triggers(self, starts, n_starts):
        if starts is None:
            if n_starts is not None:
                raise ValueError("n_starts without starts")
            return {}
        if (not isinstance(starts, torch.Tensor) or starts.dtype != torch.int64 or starts.dim() != 2
                or starts.shape[0] != self.B or starts.device != self.device):
            raise ValueError(f"starts must be an int64 tensor [{self.B}, K] on {self.device}, got "
                             f"{getattr(starts, 'shape', type(starts))} {getattr(starts, 'dtype', '')}")
        K = int(starts.shape[1])
        if n_starts is None:
            n_starts = self._all.get(K)
            if n_starts is None:
                n_starts = self._all[K] = torch.full((self.B,), K, dtype=torch.int32, device=self.device)
        elif (not isinstance(n_starts, torch.Tensor) or n_starts.dtype != torch.int32
              or tuple(n_starts.shape) != (self.B,) or n_starts.device != self.device):
            raise ValueError(f"n_starts must be an int32 tensor [{self.B}] on {self.device}")
        return dict(starts=starts, n_starts=n_starts.contiguous())

    def push(self, x: torch.Tensor, starts: torch.Tensor | None = None, n_starts: torch.Tensor | None = None,
             final: bool = False) -> FrameCaptureResult:
        """The next chunk of every stream and this call's triggers; ``final=True`` also ends the streams."""
        kw = self._triggers(starts, n_starts)
        x, Tc = self._chunk(x, final)
        return self._call(x, Tc, final, **kw)

    def push_compact(self, x: torch.Tensor, starts: torch.Tensor | None = None,
                     n_starts: torch.Tensor | None = None, final: bool = False) -> CompactFrames:
        """``push`` with the call's frames written densely (``CompactFrames``): same arguments, same state,
        same rules; never synchronises.  Needs ``compact_rows``."""
        r = self._compact
        if r is None:
            raise ValueError("push_compact needs a FrameCapture made with compact_rows")
        kw = self._triggers(starts, n_starts)
        x, Tc = self._chunk(x, final)
        rc = self._fn_compact(*self._head(x.data_ptr(), Tc, kw.get("starts"), kw.get("n_starts")), self.compact_rows,
                              r.frames.data_ptr(), r.frame_start.data_ptr(), r.frame_stream.data_ptr(),
                              r.row0.data_ptr(), r.n_rows.data_ptr(), r.n_frames.data_ptr(), r.dropped.data_ptr(),
                              int(bool(final)), _lib.stream_ptr())
        _lib.check(rc, "ofs_frame_capture_compact")
        self.samples_seen = 0 if final else self.samples_seen + Tc
        return r

    def live(self, result: FrameCaptureResult):
        """``(stream_index [n], slot [n], frames [n, n_br, F(, 2)], start [n])`` of the slots ``result``'s
        call wrote, in (stream, slot) order.  THE ONE CALL THAT SYNCHRONISES with the host (the number of
        frames sizes the tensors); ``frames`` and ``start`` are copies."""
        b, slot = torch.nonzero(result.frame_start >= 0, as_tuple=True)
        return b, slot, result.frames[b, slot], result.frame_start[b, slot]


class StreamReceiver:
    """Chunks in, decoded frames out, with no host synchronisation: ``FrameCapture.push_compact`` followed
    by the counted back-end (``core.receiver_backend_batched(..., origin=frame_start, n_active=n_rows[:1])``)
    on the rows it wrote.

    ``cap`` is a ``FrameCapture`` made with ``compact_rows``; ``pilot_offset`` / ``data_offset`` are the CP
    starts of the pilot and the data symbol relative to the frame start; ``pilot_used`` / ``data_used`` the
    known symbols, ``[n_used]`` or ``[compact_rows, n_used]`` per row; ``cfo_hz`` (optional) per row.
    ``push(x, starts, n_starts, final=False)`` returns ``(CompactFrames, dict)``: the capture's result and
    the back-end's outputs ``[compact_rows, ...]``, of which rows ``[0, n_rows[0])`` are valid (the other
    rows keep what they held).  Both are this object's buffers, overwritten in stream order by the next
    push.  ``push`` reads no device value on the host and, after the first push, allocates nothing: a
    receive loop can be enqueued ahead of the device."""

    def __init__(self, cap: FrameCapture, pilot_offset: int, data_offset: int, pilot_used, data_used, *,
                 n_fft: int, cp_len: int, fs_hz: float, bins=None, cfo_hz=None):
        if not isinstance(cap, FrameCapture) or cap.compact_rows is None:
            raise ValueError("StreamReceiver needs a FrameCapture made with compact_rows")
        self.cap = cap
        R, dev = cap.compact_rows, cap.device
        k = core.centered_subcarrier_indices(core.NUM_ACTIVE_SUBCARRIERS) if bins is None else np.asarray(bins)
        self._bins = torch.as_tensor(k.astype(np.int32)).to(dev)
        U = int(self._bins.numel())

        def known(v):
            t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.complex128))
            t = t.to(device=dev, dtype=torch.complex128).contiguous()
            if tuple(t.shape) not in ((U,), (R, U)):
                raise ValueError(f"known symbols must be [{U}] or [{R}, {U}], got {tuple(t.shape)}")
            return t

        self._pilot, self._data = known(pilot_used), known(data_used)
        # the constant per-row starts, built once
        self._ps = torch.full((R,), int(pilot_offset), dtype=torch.int64, device=dev)
        self._ds = torch.full((R,), int(data_offset), dtype=torch.int64, device=dev)
        self._cfo = None
        if cfo_hz is not None:
            c = cfo_hz if isinstance(cfo_hz, torch.Tensor) else torch.as_tensor(np.asarray(cfo_hz, np.float64))
            c = c.to(device=dev, dtype=torch.float64).reshape(-1)
            if c.numel() == 1:
                c = c.expand(R)
            if c.numel() != R:
                raise ValueError(f"cfo_hz must have one value, or one per row ({R})")
            self._cfo = c.contiguous()
        self._kw = dict(n_fft=int(n_fft), cp_len=int(cp_len), fs_hz=float(fs_hz))
        self._out = None

    def push(self, x: torch.Tensor, starts: torch.Tensor | None = None, n_starts: torch.Tensor | None = None,
             final: bool = False):
        res = self.cap.push_compact(x, starts, n_starts, final)
        self._out = core.receiver_backend_batched(res.frames, self._ps, self._ds, self._pilot, self._data,
                                                  bins=self._bins, cfo_hz=self._cfo, origin=res.frame_start,
                                                  n_active=res.n_rows[:1], out=self._out, **self._kw)
        return res, self._out
