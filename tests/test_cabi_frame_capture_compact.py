"""CPU: ofs_frame_capture_compact and ofs_rx_backend_counted reject bad arguments before any launch (no GPU
here: a call that got as far as a launch would fail differently), as test_cabi_frame_capture.py checks
the slot form."""
import ctypes
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
C64, C128, CI16, CP12 = 0, 1, 2, 3
OK, EINVAL = 0, -1
OUTPUTS = ("frames", "fs", "fstream", "row0", "n_rows", "nf", "dr")


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
          trig_max=1, state=16, cap=4, frames=16, fs=16, fstream=16, row0=16, n_rows=16, nf=16, dr=16, final=0):
    """Pointers are fake non-null addresses (16 = aligned): a valid call would launch, so only calls
    that must return before any launch are made with them."""
    return lib.ofs_frame_capture_compact(fmt, x, B, nb, Tc, F, H, Q, offset, trig, ld, stride, n_trig, trig_max,
                                         state, cap, frames, fs, fstream, row0, n_rows, nf, dr, final, None)


def test_every_einval_of_the_slot_form_holds(lib):
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
    assert _call(lib, frames=20) == EINVAL                        # complex64 frames at a 4-byte address


def test_capacity_range(lib):
    for cap in (0, -1, -(1 << 40), 1 << 31, 1 << 40):
        assert _call(lib, cap=cap) == EINVAL, cap
        assert _call(lib, cap=cap, B=0, x=None, state=None, **{o: None for o in OUTPUTS}) == EINVAL, cap


def test_each_null_output_is_refused(lib):
    for out in OUTPUTS:
        assert _call(lib, **{out: None}) == EINVAL, out


def test_empty_batch_without_outputs_is_a_no_op(lib):
    none = {o: None for o in OUTPUTS}
    assert _call(lib, B=0, x=None, state=None, trig=None, n_trig=None, **none) == OK
    assert _call(lib, B=0, x=None, state=None, trig=None, n_trig=None, cap=(1 << 31) - 1, **none) == OK
    assert _call(lib, B=0, Tc=0, final=1, **none) == OK
    assert _call(lib, B=0, Tc=0, final=0, **none) == EINVAL
    assert _call(lib, B=0, Q=17, **none) == EINVAL


def test_the_state_size_function_is_shared(lib):
    """One size function, one state layout: the compact form has none of its own."""
    assert lib.ofs_frame_capture_state_bytes(C64, 2, 7, 44, 3) == 192 + 2 * 44 * 8
    for name in ("ofs_frame_capture_compact_state_bytes", "ofs_frame_capture_compact_max_samples"):
        with pytest.raises(AttributeError):
            getattr(lib, name)
    # what the size function refuses, the compact form refuses (and the slot form: test_cabi_frame_capture.py)
    for nb, F, H, Q in ((0, 4, 4, 2), (1, 0, 4, 2), (1, 5, 4, 2), (1, 4, 4, 0), (1, 4, 4, 17), (1, 4, 1 << 30, 2)):
        assert lib.ofs_frame_capture_state_bytes(C64, nb, F, H, Q) < 0
        assert _call(lib, nb=nb, F=F, H=H, Q=Q) == EINVAL, (nb, F, H, Q)


def test_backend_counted_refusals(lib):
    def call(origin, n_active, n_fft=256, x=16, ps=16):
        return lib.ofs_rx_backend_counted(C64, x, 1, 1, 1024, n_fft, 64, 1e6, ps, 16, None, 8, 16, 16, 0, 16, 0,
                                          None, None, None, None, None, None, None, None, origin, n_active, None)
    assert call(None, 16) == EINVAL                               # a count without an origin
    assert call(None, 16, x=None) == EINVAL
    for origin, n_active in ((16, 16), (16, None), (None, None)):  # and what the back-end refuses
        assert call(origin, n_active, n_fft=255) == EINVAL
        assert call(origin, n_active, x=None) == EINVAL
        assert call(origin, n_active, ps=None) == EINVAL
