"""Host scaffolding shared by the resumable chunk-fed detectors and metrics (``ofs_*_chunk*``).

``ChunkedStreams`` owns what they have in common: the per-stream device state (all-zero = fresh), the
host count of samples taken in, the result buffers cached per ``Tc``, the library call with its status
check, ``push`` / ``flush`` / ``reset``.  A subclass names its C entry points (``_entry``, ``_sizes``) and
supplies ``_chunk`` (one of the validators below), ``_alloc`` and ``_launch``.
"""
from __future__ import annotations

import torch

from . import _lib


def _checked(det, x: torch.Tensor, Tc: int, final: bool, shape_note: str = ""):
    """The checks behind every validator: ``max_chunk``, the empty chunk, the device move."""
    if det.max_chunk is not None and Tc > det.max_chunk:
        raise ValueError(f"chunk of {Tc} samples exceeds max_chunk = {det.max_chunk}{shape_note}; push it in pieces")
    if Tc == 0 and not final:
        raise ValueError("an empty chunk is only valid with final=True (or flush())")
    if x.device != det.device:
        x = x.to(det.device)
    return x.contiguous(), Tc


def complex_chunk(det, x, final: bool, n_branch: int, dtype, type_name: str | None = None):
    """Validate a complex / IQ chunk for ``det`` (before any library call): ``[B, n_branch, Tc]`` of
    ``dtype`` (int16: a trailing I/Q axis of 2), or without the branch axis for one branch.  Returns the
    contiguous device tensor ``[B, n_branch, Tc(, 2)]`` and ``Tc``."""
    iq = (2,) if dtype == torch.int16 else ()
    tail = ", 2" if iq else ""
    what = (f"[{det.B}, {n_branch}, Tc{tail}] {type_name or dtype}" +
            (f" (or [{det.B}, Tc{tail}])" if n_branch == 1 else ""))
    if not isinstance(x, torch.Tensor) or x.dtype != dtype:
        raise ValueError(f"chunk must be {what}, got dtype {getattr(x, 'dtype', type(x))}")
    if x.dim() == 2 + len(iq) and n_branch == 1:
        x = x[:, None]
    if x.dim() != 3 + len(iq) or x.shape[0] != det.B or x.shape[1] != n_branch or tuple(x.shape[3:]) != iq:
        raise ValueError(f"chunk must be {what}, got {tuple(x.shape)} {x.dtype}")
    return _checked(det, x, int(x.shape[2]), final)


def word_chunk(det, x, final: bool, n_branch: int, shape_note: str):
    """Validate an integer detector chunk for ``det`` (before any library call): int16
    ``[B, n_branch, Tc, 2]``, or for ``det.fmt == CP12`` packed 12-bit words ``[B, Tc, 3 * n_branch]`` uint8.
    ``shape_note`` ends the ``max_chunk`` message.  Returns the contiguous device tensor and ``Tc``."""
    if det.fmt == _lib.CP12:
        ok = x.dtype == torch.uint8 and x.dim() == 3 and x.shape[0] == det.B and x.shape[2] == 3 * n_branch
        Tc = int(x.shape[1]) if ok else 0
        what = f"[{det.B}, Tc, {3 * n_branch}] uint8"
    else:
        ok = (x.dtype == torch.int16 and x.dim() == 4 and x.shape[0] == det.B and x.shape[1] == n_branch
              and x.shape[3] == 2)
        Tc = int(x.shape[2]) if ok else 0
        what = f"[{det.B}, {n_branch}, Tc, 2] int16"
    if not ok:
        raise ValueError(f"chunk must be {what}, got {tuple(x.shape)} {x.dtype}")
    return _checked(det, x, Tc, final, shape_note)


def word_format(in_dtype) -> int:
    """The input format of an integer detector: ``torch.int16`` or ``"cp12"``."""
    if in_dtype == "cp12":
        return _lib.CP12
    if in_dtype == torch.int16:
        return _lib.CI16
    raise ValueError(f'in_dtype must be torch.int16 or "cp12", got {in_dtype!r}')


class ChunkedStreams:
    """B resumable streams: ``state`` ``[B, nbytes]`` uint8 on the device, ``max_chunk`` (the largest
    ``Tc`` of one call, None where the call has no limit), ``samples_seen`` (host count of samples pushed
    since the last full reset / final call).  Subclasses set ``_entry`` (the chunk call) and ``_sizes``
    (the prefix of its ``_state_bytes`` / ``_max_samples`` functions) and define
    ``_chunk(x, final) -> (x, Tc)``, ``_alloc(Tc)`` (the result buffers of one chunk length) and
    ``_launch(x_ptr, Tc, final, buffers, **kw) -> status``."""
    _entry = _sizes = ""

    def __init__(self, B: int, device, size_args: tuple, supports: str):
        dev = torch.device(device) if device is not None else _lib.require_gpu()
        lib = _lib.lib()
        nbytes = int(getattr(lib, self._sizes + "_state_bytes")(*size_args))
        if nbytes < 0 or B < 0:
            raise ValueError(supports)
        self.B, self.device = int(B), dev
        max_samples = getattr(lib, self._sizes + "_max_samples", None)          # (zc_chunk has no limit)
        self.max_chunk = int(max_samples(*size_args)) if max_samples else None
        self.state = torch.zeros((self.B, nbytes), dtype=torch.uint8, device=dev)     # all-zero = fresh
        self.samples_seen = 0
        self._fn = getattr(lib, self._entry)
        self._bufs: dict = {}

    def _buffers(self, Tc: int, *key):
        """The cached buffers of chunk length ``Tc`` (and kind of call ``key``, where a class has several)."""
        k = (*key, Tc) if key else Tc
        r = self._bufs.get(k)
        if r is None:
            r = self._bufs[k] = self._alloc(Tc)
        return r

    def _call(self, x, Tc: int, final: bool, *key, **kw):
        r = self._buffers(Tc, *key)
        rc = self._launch(None if x is None else x.data_ptr(), Tc, int(bool(final)), r, **kw)
        _lib.check(rc, self._entry)
        self.samples_seen = 0 if final else self.samples_seen + Tc
        return r

    def push(self, x: torch.Tensor, final: bool = False):
        """The next chunk of every stream; ``final=True`` also ends the streams (open gates close where
        the detector closes them at a stream's end; fresh afterwards)."""
        x, Tc = self._chunk(x, final)
        return self._call(x, Tc, final)

    def flush(self):
        """End the streams without new samples: the per-sample outputs are None, the rest is written as
        by a final push; the streams are fresh afterwards."""
        return self._call(None, 0, True)

    def reset(self, mask: torch.Tensor | None = None) -> None:
        """Make all streams fresh, or those where ``mask`` [B] (bool) is set, without closing their
        gates (stream-ordered, no synchronisation).  ``samples_seen`` restarts only on a full reset."""
        if mask is None:
            self.state.zero_()
            self.samples_seen = 0
        else:
            m = torch.as_tensor(mask, dtype=torch.bool).to(self.device)
            self.state.masked_fill_(m[:, None], 0)
