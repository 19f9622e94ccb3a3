"""CPU: ofs_zc_freq_metric_chunk and its size functions reject bad arguments before any launch (no GPU
here: a call that got as far as a launch would fail differently), as test_cabi_park_chunk.py checks
the Park call."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
C64, C128, CI16, CP12 = 0, 1, 2, 3
FP32, FP64 = 0, 1
OK, EINVAL = 0, -1

IDX = np.array([-2, -1, 1, 2], dtype=np.int32)              # host template (read before any launch)
TB = np.array([1, 1j, -1, 0.5 - 0.5j], dtype=np.complex128)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build_hip()
    from ofdm_sync_amd import _lib as L
    l = ctypes.CDLL(LIB)
    L._declare(l)
    return l


def _call(lib, fmt=C64, x=16, B=1, nb=1, Tc=8, N=64, cp=0, prec=FP32, nbins=4, idx=IDX.ctypes.data,
          tb=TB.ctypes.data, state=16, metric=16, off0=None, pi=None, pv=None, final=0):
    """Device pointers are fake non-null addresses (16 = aligned): a valid call would launch, so only
    calls that must return before any launch are made with them."""
    return lib.ofs_zc_freq_metric_chunk(fmt, x, B, nb, Tc, N, cp, prec, nbins, idx, tb, 3.25, state, metric, off0,
                                        pi, pv, final, None)


def test_every_einval_is_returned_before_any_launch(lib):
    # format / precision pairs other than (C64, FP32), (C128, FP64), (CI16, FP64)
    for fmt, prec in ((C64, FP64), (C128, FP32), (CI16, FP32), (CP12, FP64), (CP12, FP32), (7, FP32), (C64, 9),
                      (-1, FP32)):
        assert _call(lib, fmt=fmt, prec=prec) == EINVAL, (fmt, prec)
    # branches: the sliding kernel takes 1 or 2 (3-4 go to the older kernel in the one-shot call)
    for nb in (0, -1, 3, 4, 5):
        assert _call(lib, nb=nb) == EINVAL, nb
    # N: at least 64, a multiple of 64, the blocks of a window within LDS
    for N in (0, -64, 1, 32, 63, 65, 96, 100, 2000, 2048 + 32, 10304, 1 << 20):
        assert _call(lib, N=N) == EINVAL, N
    assert _call(lib, cp=-1) == EINVAL
    # the template: 1..64 bins, host pointers
    for nbins in (0, -1, 65):
        assert _call(lib, nbins=nbins) == EINVAL, nbins
    assert _call(lib, idx=None) == EINVAL
    assert _call(lib, tb=None) == EINVAL
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
    # the peak advances only with the metric: asking for it without one and with samples
    assert _call(lib, metric=None, pi=16) == EINVAL
    assert _call(lib, metric=None, pv=16) == EINVAL
    assert _call(lib, metric=None, off0=16, pi=16, pv=16, final=1) == EINVAL


def test_empty_batch_is_a_no_op(lib):
    assert _call(lib, B=0) == OK
    assert _call(lib, B=0, x=None, state=None, metric=None, final=1) == OK
    assert _call(lib, B=0, x=None, state=None, metric=None, Tc=0, final=1) == OK
    assert _call(lib, B=0, x=None, state=None, metric=None, fmt=CI16, prec=FP64, N=2048, cp=512, nb=2) == OK
    assert _call(lib, B=0, Tc=0, final=0) == EINVAL              # Tc = 0 without final stays an error
    assert _call(lib, B=0, fmt=C64, prec=FP64) == EINVAL
    assert _call(lib, B=0, nb=3) == EINVAL


def test_size_functions(lib):
    sizes = {}
    for fmt, sample in ((C64, 8), (C128, 16), (CI16, 4)):
        for nb in (1, 2):
            for N, cp in ((64, 0), (128, 9), (192, 16), (256, 64), (2048, 512), (4096, 0), (8192, 0), (4160, 7)):
                n = lib.ofs_zc_freq_chunk_state_bytes(fmt, nb, N, cp)
                # a header and at least the N + 64 - 2 samples before a chunk that a call may read
                assert n > 0 and n % 16 == 0 and n >= nb * (N + 62) * sample, (fmt, nb, N, cp, n)
                assert n <= 64 + nb * (N + 256) * sample, (fmt, nb, N, cp, n)
                assert lib.ofs_zc_freq_chunk_max_samples(fmt, nb, N, cp) == 1 << 30
                sizes[fmt, nb, N] = n
        for nb, N, cp in ((0, 64, 0), (-1, 64, 0), (3, 64, 0), (4, 2048, 512), (1, 0, 0), (1, 32, 0), (1, 100, 0),
                          (1, 2000, 0), (1, -64, 0), (1, 10304, 0), (1, 1 << 20, 0), (1, 64, -1)):
            assert lib.ofs_zc_freq_chunk_state_bytes(fmt, nb, N, cp) < 0, (fmt, nb, N, cp)
            assert lib.ofs_zc_freq_chunk_max_samples(fmt, nb, N, cp) < 0, (fmt, nb, N, cp)
    for fmt in (CP12, 4, -1):
        assert lib.ofs_zc_freq_chunk_state_bytes(fmt, 1, 64, 0) < 0
        assert lib.ofs_zc_freq_chunk_max_samples(fmt, 1, 64, 0) < 0
    # grows with N and n_br, and by the sample size with the format (the header is 64 bytes)
    for fmt in (C64, C128, CI16):
        assert sizes[fmt, 1, 64] < sizes[fmt, 1, 128] < sizes[fmt, 1, 2048] < sizes[fmt, 1, 8192]
        for N in (64, 2048, 8192):
            assert sizes[fmt, 2, N] - 64 == 2 * (sizes[fmt, 1, N] - 64)
    for nb in (1, 2):
        for N in (64, 2048, 8192):
            assert sizes[C128, nb, N] - 64 == 2 * (sizes[C64, nb, N] - 64) == 4 * (sizes[CI16, nb, N] - 64)
