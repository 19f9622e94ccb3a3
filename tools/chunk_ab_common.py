"""Helpers shared by the chunked-against-one-shot timing tools (tools/*_chunk_ab.py)."""
import torch


def timed(fn, steps, st):
    """Mean milliseconds of one ``fn()`` over ``steps`` calls enqueued on stream ``st``, between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(steps):
        fn()
    e1.record(st)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def bits(t):
    """``t`` as integers of its elements' width (complex: a trailing real / imaginary axis), for
    bit-for-bit comparisons that NaNs and signed zeros do not fool."""
    t = (torch.view_as_real(t) if t.is_complex() else t).contiguous()
    return t.view(torch.int64 if t.element_size() == 8 else torch.int32)
