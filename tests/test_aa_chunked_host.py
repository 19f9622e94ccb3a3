"""CPU: the chunked [A][A] entry points (include/ofdmsync.h, ofs_aa_detect_chunk) size their state
and reject bad arguments before any GPU call.  No launch happens here."""
import ctypes
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
LS = (64, 128, 256, 512, 1024)
CI16, CP12, EINVAL = 2, 3, -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build_hip()
    from ofdm_sync_amd import _lib as L
    l = ctypes.CDLL(LIB)
    L._declare(l)
    return l


def test_state_bytes_positive_multiple_of_16_and_grows_with_antennas(lib):
    for L in LS:
        one, two = lib.ofs_aa_chunk_state_bytes(1, L), lib.ofs_aa_chunk_state_bytes(2, L)
        assert one > 0 and one % 16 == 0, (L, one)
        assert two > one and two % 16 == 0, (L, two)
        assert one >= 2 * L * 4                        # at least the last 2L int16 I/Q words


def test_state_bytes_rejects_unsupported_shapes(lib):
    assert lib.ofs_aa_chunk_state_bytes(1, 96) < 0
    assert lib.ofs_aa_chunk_state_bytes(3, 128) < 0
    assert lib.ofs_aa_chunk_state_bytes(0, 128) < 0
    assert lib.ofs_aa_chunk_max_samples(1, 96) < 0
    assert lib.ofs_aa_chunk_max_samples(3, 128) < 0


def test_max_samples(lib):
    for n_ant in (1, 2):
        for L in LS:
            assert lib.ofs_aa_chunk_max_samples(n_ant, L) == (1 << 21) // n_ant - 2 * L


def _call(lib, fmt=CI16, x=16, B=1, n_ant=1, Tc=256, L=128, state=16, detect=0, max_events=0, n_events=None,
          ev_int=None, ev_real=None, final=0, hysteresis=16):
    """ofs_aa_detect_chunk with small non-null integers standing in for device pointers: every case
    below must be refused before anything is dereferenced or launched."""
    return lib.ofs_aa_detect_chunk(fmt, x, B, n_ant, Tc, L, state, None, None, None, None, detect, 0.15, hysteresis,
                                   15.36e6, max_events, n_events, ev_int, ev_real, final, None)


def test_argument_validation_without_gpu(lib):
    """Each case of the header's OFS_EINVAL list returns it (before any HIP call)."""
    for fmt in (0, 1, 7):                                              # complex64 / complex128 / unknown
        assert _call(lib, fmt=fmt) == EINVAL
    assert _call(lib, n_ant=0) == EINVAL
    assert _call(lib, n_ant=3) == EINVAL
    for L in (0, 96, 192, 2048):
        assert _call(lib, L=L) == EINVAL
    for n_ant in (1, 2):
        for L in LS:
            cap = lib.ofs_aa_chunk_max_samples(n_ant, L)
            assert _call(lib, n_ant=n_ant, L=L, Tc=cap + 1) == EINVAL
    assert _call(lib, Tc=0, final=0) == EINVAL                         # empty chunk that is no flush
    assert _call(lib, Tc=-1, final=1) == EINVAL
    assert _call(lib, B=-1) == EINVAL
    assert _call(lib, state=None) == EINVAL                            # null state with B > 0
    assert _call(lib, state=None, Tc=0, final=1) == EINVAL             # ... also for a flush
    assert _call(lib, state=8) == EINVAL                               # state not 16-byte aligned
    assert _call(lib, x=None) == EINVAL                                # null samples with B * Tc > 0
    assert _call(lib, detect=1, max_events=4, n_events=None, ev_int=16, ev_real=16) == EINVAL
    assert _call(lib, detect=1, max_events=4, n_events=16, ev_int=None, ev_real=16) == EINVAL
    assert _call(lib, detect=1, max_events=4, n_events=16, ev_int=16, ev_real=None) == EINVAL
    assert _call(lib, detect=1, max_events=-1, n_events=16) == EINVAL
    assert _call(lib, fmt=CP12, n_ant=3) == EINVAL
    assert _call(lib, hysteresis=(1 << 28) + 1) == EINVAL              # OFS_AA_CHUNK_MAX_HYSTERESIS


def test_empty_batch_is_a_valid_no_op(lib):
    """B = 0 launches nothing and every pointer may be null."""
    assert _call(lib, B=0, x=None, state=None) == 0
    assert _call(lib, B=0, x=None, state=None, Tc=0, final=1, detect=1, max_events=4) == 0
