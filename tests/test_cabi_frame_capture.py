"""CPU: ofs_frame_capture_chunk, its size function and ofs_rx_backend_at reject bad arguments before any
launch (no GPU here: a call that got as far as a launch would fail differently), as test_cabi.py checks
the others."""
import ctypes
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
C64, C128, CI16, CP12 = 0, 1, 2, 3
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


def _call(lib, fmt=C64, x=16, B=1, nb=1, Tc=8, F=4, H=4, Q=2, offset=0, trig=16, ld=1, stride=1, n_trig=16,
          trig_max=1, state=16, frames=16, fs=16, nf=16, dr=16, final=0):
    """Pointers are fake non-null addresses (16 = aligned): a valid call would launch, so only calls
    that must return before any launch are made with them."""
    return lib.ofs_frame_capture_chunk(fmt, x, B, nb, Tc, F, H, Q, offset, trig, ld, stride, n_trig, trig_max,
                                       state, frames, fs, nf, dr, final, None)


def test_every_einval_is_returned_before_any_launch(lib):
    for fmt in (CP12, 4, -1):
        assert _call(lib, fmt=fmt) == EINVAL, fmt
    assert _call(lib, nb=0) == EINVAL
    assert _call(lib, F=0) == EINVAL and _call(lib, F=-3) == EINVAL
    assert _call(lib, F=5, H=4) == EINVAL                         # history < frame_len
    assert _call(lib, H=1 << 30) == EINVAL                        # above the limit
    assert _call(lib, Q=0) == EINVAL and _call(lib, Q=17) == EINVAL and _call(lib, Q=-1) == EINVAL
    assert _call(lib, Tc=-1) == EINVAL
    assert _call(lib, Tc=0, final=0) == EINVAL
    assert _call(lib, B=-1) == EINVAL
    assert _call(lib, state=None) == EINVAL and _call(lib, state=24) == EINVAL and _call(lib, state=4) == EINVAL
    assert _call(lib, x=None) == EINVAL
    assert _call(lib, trig_max=-1) == EINVAL
    assert _call(lib, trig=None) == EINVAL                        # triggers announced, none given
    for out in ("frames", "fs", "nf", "dr"):
        assert _call(lib, **{out: None}) == EINVAL, out
    assert _call(lib, frames=20) == EINVAL                        # complex64 frames at a 4-byte address


def test_empty_batch_is_a_no_op(lib):
    assert _call(lib, B=0) == OK
    assert _call(lib, B=0, x=None, state=None, frames=None, fs=None, nf=None, dr=None, trig=None, n_trig=None) == OK
    assert _call(lib, B=0, Tc=0, final=1) == OK
    assert _call(lib, B=0, Tc=0, final=0) == EINVAL
    assert _call(lib, B=0, Q=17) == EINVAL


def test_size_function(lib):
    for fmt, sample in ((C64, 8), (C128, 16), (CI16, 4)):
        for nb in (1, 2, 3):
            for F, H in ((1, 1), (7, 7), (7, 44), (64, 128), (300, 337), (8192, 8192), (1, (1 << 30) - 4)):
                for Q in (1, 2, 16):
                    n = lib.ofs_frame_capture_state_bytes(fmt, nb, F, H, Q)
                    assert n % 16 == 0 and nb * H * sample <= n - 192 < nb * (H * sample + 16), (fmt, nb, F, H, Q, n)
        for bad in ((0, 4, 4, 2), (1, 0, 4, 2), (1, 5, 4, 2), (1, 4, 4, 0), (1, 4, 4, 17), (1, 4, 1 << 30, 2)):
            assert lib.ofs_frame_capture_state_bytes(fmt, *bad) < 0, (fmt, bad)
    for fmt in (CP12, 4, -1):
        assert lib.ofs_frame_capture_state_bytes(fmt, 1, 4, 4, 2) < 0
    with pytest.raises(AttributeError):
        lib.ofs_frame_capture_max_samples                        # no chunk limit, so no such function


def test_backend_at_refuses_what_the_backend_refuses(lib):
    def call(fn, extra, n_fft=256, x=16, ps=16):
        return fn(C64, x, 1, 1, 1024, n_fft, 64, 1e6, ps, 16, None, 8, 16, 16, 0, 16, 0, None, None, None, None,
                  None, None, None, None, *extra, None)
    for fn, extra in ((lib.ofs_rx_backend, ()), (lib.ofs_rx_backend_at, (None,)), (lib.ofs_rx_backend_at, (16,))):
        assert call(fn, extra, n_fft=255) == EINVAL
        assert call(fn, extra, x=None) == EINVAL
        assert call(fn, extra, ps=None) == EINVAL
