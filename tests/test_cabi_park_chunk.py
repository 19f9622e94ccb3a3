"""CPU: ofs_park_metric_chunk and its size functions reject bad arguments before any launch (no GPU
here: a call that got as far as a launch would fail differently), as test_cabi.py checks the others."""
import ctypes
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
C64, C128, CI16, CP12 = 0, 1, 2, 3
FP32, FP64 = 0, 1
OK, EINVAL = 0, -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build_hip()
    from ofdm_sync_amd import _lib as L
    l = ctypes.CDLL(LIB)
    L._declare(l)
    return l


def _call(lib, fmt=C64, x=16, B=1, nb=1, Tc=8, N=64, prec=FP32, state=16, M=16, P=None, E=None, d0=None,
          pi=None, pv=None, final=0):
    """Pointers are fake non-null addresses (16 = aligned): a valid call would launch, so only calls
    that must return before any launch are made with them."""
    return lib.ofs_park_metric_chunk(fmt, x, B, nb, Tc, N, prec, state, M, P, E, d0, pi, pv, final, None)


def test_every_einval_is_returned_before_any_launch(lib):
    # format / precision pairs other than (C64, FP32), (C128, FP64), (CI16, FP64)
    for fmt, prec in ((C64, FP64), (C128, FP32), (CI16, FP32), (CP12, FP64), (CP12, FP32), (7, FP32), (C64, 9),
                      (-1, FP32)):
        assert _call(lib, fmt=fmt, prec=prec) == EINVAL, (fmt, prec)
    # branches, half < 1, the LDS limit of the one-shot call
    assert _call(lib, nb=0) == EINVAL
    assert _call(lib, nb=-1) == EINVAL
    for N in (1, 0, -2):
        assert _call(lib, N=N) == EINVAL, N
    assert _call(lib, N=8191) == EINVAL
    assert _call(lib, N=8192) == EINVAL
    assert _call(lib, fmt=C128, prec=FP64, N=4095) == EINVAL
    assert _call(lib, fmt=CI16, prec=FP64, N=4096) == EINVAL
    # Tc: negative, above the limit, 0 without final
    assert _call(lib, Tc=-1) == EINVAL
    assert _call(lib, Tc=(1 << 30) + 1) == EINVAL
    assert _call(lib, Tc=0, final=0) == EINVAL
    # B < 0
    assert _call(lib, B=-1) == EINVAL
    # state: null or misaligned with B > 0
    assert _call(lib, state=None) == EINVAL
    assert _call(lib, state=None, Tc=0, final=1) == EINVAL
    assert _call(lib, state=24) == EINVAL
    assert _call(lib, state=4) == EINVAL
    # x: null with B * Tc > 0
    assert _call(lib, x=None) == EINVAL
    # the peak advances only with M: asking for it without M and with samples
    assert _call(lib, M=None, pi=16) == EINVAL
    assert _call(lib, M=None, pv=16) == EINVAL
    assert _call(lib, M=None, P=16, E=16, pi=16, pv=16, final=1) == EINVAL


def test_empty_batch_is_a_no_op(lib):
    assert _call(lib, B=0) == OK
    assert _call(lib, B=0, x=None, state=None, M=None, final=1) == OK
    assert _call(lib, B=0, x=None, state=None, M=None, Tc=0, final=1) == OK
    assert _call(lib, B=0, x=None, state=None, M=None, pi=None, pv=None, fmt=CI16, prec=FP64, N=4094, nb=3) == OK
    assert _call(lib, B=0, Tc=0, final=0) == EINVAL              # Tc = 0 without final stays an error
    assert _call(lib, B=0, fmt=C64, prec=FP64) == EINVAL


def test_size_functions(lib):
    for fmt, sample, nmax in ((C64, 8, 8190), (C128, 16, 4094), (CI16, 4, 4094)):
        for nb in (1, 2, 3):
            for N in (2, 3, 8, 30, 64, 2048, nmax - 1, nmax):
                n = lib.ofs_park_chunk_state_bytes(fmt, nb, N)
                half = N // 2
                # a header and at least the 2 * half + 6 samples before a chunk that a call reads
                assert n > 0 and n % 16 == 0 and n >= nb * (2 * half + 6) * sample, (fmt, nb, N, n)
                assert lib.ofs_park_chunk_max_samples(fmt, nb, N) == 1 << 30
        for nb, N in ((0, 64), (-1, 64), (1, 1), (1, 0), (1, -4), (1, nmax + 1), (1, 1 << 20)):
            assert lib.ofs_park_chunk_state_bytes(fmt, nb, N) < 0, (fmt, nb, N)
            assert lib.ofs_park_chunk_max_samples(fmt, nb, N) < 0, (fmt, nb, N)
    for fmt in (CP12, 4, -1):
        assert lib.ofs_park_chunk_state_bytes(fmt, 1, 64) < 0
        assert lib.ofs_park_chunk_max_samples(fmt, 1, 64) < 0
