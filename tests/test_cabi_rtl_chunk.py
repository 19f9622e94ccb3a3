"""CPU: the chunked minn_rtl entry points (include/ofdmsync.h, ofs_minn_rtl_chunk) are declared and
exported, size their state and reject bad arguments before any GPU call.  No launch happens here."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
HDR = os.path.join(ROOT, "include", "ofdmsync.h")
QS = (64, 128, 256, 512)
CI16, CP12, EINVAL = 2, 3, -1
SYMBOLS = ("ofs_rtl_chunk_state_bytes", "ofs_rtl_chunk_max_samples", "ofs_minn_rtl_chunk")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build_hip()
    from ofdm_sync_amd import _lib as L
    l = ctypes.CDLL(LIB)
    L._declare(l)
    return l


def test_symbols_declared_in_the_header_and_exported(lib):
    text = open(HDR).read()
    for name in SYMBOLS:
        assert re.search(r"\bint(32|64)_t\s+" + name + r"\s*\(", text), name
        assert getattr(lib, name) is not None
    assert "OFS_RTL_CHUNK_MAX_HYSTERESIS" in text and "EQUIVALENCE GUARANTEE" in text


def test_state_bytes_and_max_samples_on_the_table(lib):
    for nb in (1, 2):
        for Q in QS:
            n = lib.ofs_rtl_chunk_state_bytes(nb, Q)
            assert n > 0 and n % 16 == 0, (nb, Q, n)
            assert n >= 3 * Q * nb * 4                 # at least the last 3Q int16 I/Q words per branch
            assert lib.ofs_rtl_chunk_max_samples(nb, Q) == (1 << 21) // nb - 3 * Q
        assert lib.ofs_rtl_chunk_state_bytes(2, 64) > lib.ofs_rtl_chunk_state_bytes(1, 64)


def test_sizes_reject_shapes_off_the_table(lib):
    for nb, Q in ((1, 96), (1, 192), (1, 1024), (1, 0), (1, -64), (0, 64), (3, 64), (4, 128)):
        assert lib.ofs_rtl_chunk_state_bytes(nb, Q) == EINVAL, (nb, Q)
        assert lib.ofs_rtl_chunk_max_samples(nb, Q) == EINVAL, (nb, Q)


def _call(lib, fmt=CI16, x=16, B=1, n_br=1, Tc=256, Q=128, shift=3, mode=0, frac=15, state=16, detect=0,
          hysteresis=2, max_events=0, n_events=None, events=None, open_start=None, final=0):
    """ofs_minn_rtl_chunk with small non-null integers standing in for device pointers: every case
    below must be refused before anything is dereferenced or launched."""
    return lib.ofs_minn_rtl_chunk(fmt, x, B, n_br, Tc, Q, shift, mode, 3276, frac, state, None, None, None, None,
                                  None, None, None, None, detect, hysteresis, 0, max_events, n_events, events,
                                  open_start, final, None)


def test_argument_validation_without_gpu(lib):
    """Each case of the header's OFS_EINVAL list returns it (before any HIP call)."""
    for fmt in (0, 1, 7):                                              # complex64 / complex128 / unknown
        assert _call(lib, fmt=fmt) == EINVAL
    for fmt in (CI16, CP12):
        for nb in (0, 3, 4):
            assert _call(lib, fmt=fmt, n_br=nb) == EINVAL
    for Q in (0, 96, 192, 1024):
        assert _call(lib, Q=Q) == EINVAL
    for nb in (1, 2):
        for Q in QS:
            cap = lib.ofs_rtl_chunk_max_samples(nb, Q)
            assert _call(lib, n_br=nb, Q=Q, Tc=cap + 1) == EINVAL
    assert _call(lib, Tc=0, final=0) == EINVAL                         # empty chunk that is no flush
    assert _call(lib, Tc=-1, final=1) == EINVAL
    assert _call(lib, B=-1) == EINVAL
    assert _call(lib, state=None) == EINVAL                            # null state with B > 0
    assert _call(lib, state=None, Tc=0, final=1) == EINVAL             # ... also for a flush
    assert _call(lib, state=8) == EINVAL                               # state not 16-byte aligned
    assert _call(lib, x=None) == EINVAL                                # null samples with B * Tc > 0
    assert _call(lib, shift=-1) == EINVAL                              # as ofs_minn_rtl: 0 .. 62
    assert _call(lib, shift=63) == EINVAL
    assert _call(lib, mode=2) == EINVAL
    assert _call(lib, mode=-1) == EINVAL
    assert _call(lib, hysteresis=-1) == EINVAL
    assert _call(lib, hysteresis=(1 << 28) + 1) == EINVAL              # OFS_RTL_CHUNK_MAX_HYSTERESIS
    assert _call(lib, detect=1, max_events=4, n_events=None, events=16, open_start=16) == EINVAL
    assert _call(lib, detect=1, max_events=4, n_events=16, events=16, open_start=None) == EINVAL
    assert _call(lib, detect=1, max_events=4, n_events=16, events=None, open_start=16) == EINVAL


def test_empty_batch_is_a_valid_no_op(lib):
    """B = 0 launches nothing and every pointer may be null."""
    assert _call(lib, B=0, x=None, state=None) == 0
    assert _call(lib, B=0, x=None, state=None, Tc=0, final=1, detect=1, max_events=4) == 0
