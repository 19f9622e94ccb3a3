"""CPU: the complex64 chunked [A][A] entry points (include/ofdmsync.h, ofs_aa_detect_chunk_f32) size
their state and reject bad arguments before any GPU call, and AAChunkedDetectorF32 names the chunk it
expects.  No launch happens here."""
import ctypes
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
LS = (128, 256, 512, 1024)
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build_hip()
    from ofdm_sync_amd import _lib as L
    l = ctypes.CDLL(LIB)
    L._declare(l)
    return l


def test_symbols_exported(lib):
    for name in ("ofs_aa_chunk_f32_state_bytes", "ofs_aa_chunk_f32_max_samples", "ofs_aa_detect_chunk_f32"):
        assert hasattr(lib, name), name


def test_state_bytes_multiple_of_16_and_holds_the_history(lib):
    for L in LS:
        one, two = lib.ofs_aa_chunk_f32_state_bytes(1, L), lib.ofs_aa_chunk_f32_state_bytes(2, L)
        assert one > 0 and one % 16 == 0, (L, one)
        assert two > one and two % 16 == 0, (L, two)
        assert one >= (2 * L + 127) * 8                # at least 2L + (n_seen mod 128) complex64 samples
        assert two - one >= (2 * L + 127) * 8


def test_state_bytes_rejects_unsupported_shapes(lib):
    for L in (64, 192, 2048):
        assert lib.ofs_aa_chunk_f32_state_bytes(1, L) < 0, L
        assert lib.ofs_aa_chunk_f32_max_samples(1, L) < 0, L
    for n_ant in (0, 3):
        assert lib.ofs_aa_chunk_f32_state_bytes(n_ant, 128) < 0, n_ant
        assert lib.ofs_aa_chunk_f32_max_samples(n_ant, 128) < 0, n_ant


def test_max_samples_keeps_in_call_positions_in_32_bits(lib):
    """history (2L + 127) + chunk + gate offset (hysteresis cap rounded up to a row) < 2^31."""
    for n_ant in (1, 2):
        for L in LS:
            cap = lib.ofs_aa_chunk_f32_max_samples(n_ant, L)
            assert cap >= 1 << 20
            assert 2 * L + 127 + cap + (1 << 28) + 128 < 1 << 31


def _call(lib, x=16, B=1, n_ant=1, Tc=256, L=128, state=16, detect=0, max_events=0, n_events=None,
          ev_int=None, ev_real=None, final=0, hysteresis=16):
    """ofs_aa_detect_chunk_f32 with small non-null integers standing in for device pointers: every
    case below must be refused before anything is dereferenced or launched."""
    return lib.ofs_aa_detect_chunk_f32(x, B, n_ant, Tc, L, state, None, None, None, None, detect, 0.15, hysteresis,
                                       15.36e6, max_events, n_events, ev_int, ev_real, final, None)


def test_argument_validation_without_gpu(lib):
    """Each case of the header's OFS_EINVAL list returns it (before any HIP call)."""
    assert _call(lib, n_ant=0) == EINVAL
    assert _call(lib, n_ant=3) == EINVAL
    for L in (0, 64, 96, 192, 2048):
        assert _call(lib, L=L) == EINVAL
    for n_ant in (1, 2):
        for L in LS:
            cap = lib.ofs_aa_chunk_f32_max_samples(n_ant, L)
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
    assert _call(lib, hysteresis=(1 << 28) + 1) == EINVAL              # OFS_AA_CHUNK_MAX_HYSTERESIS


def test_empty_batch_is_a_valid_no_op(lib):
    """B = 0 launches nothing and every pointer may be null."""
    assert _call(lib, B=0, x=None, state=None) == 0
    assert _call(lib, B=0, x=None, state=None, Tc=0, final=1, detect=1, max_events=4) == 0


def test_integer_entry_point_still_refuses_complex64(lib):
    """ofs_aa_detect_chunk is unchanged: complex64 (format 0) is not its input."""
    assert lib.ofs_aa_detect_chunk(0, 16, 1, 1, 256, 128, 16, None, None, None, None, 0, 0.15, 16, 15.36e6, 0, None,
                                   None, None, 0, None) == EINVAL


def test_python_names_the_expected_chunk(lib):
    """Wrong dtype or shape: a ValueError that says what a chunk looks like (raised before any launch)."""
    torch = pytest.importorskip("torch")
    from ofdm_sync_amd import sync_aa
    det = sync_aa.AAChunkedDetectorF32(2, 1, 128, device="cpu")
    assert det.max_chunk == lib.ofs_aa_chunk_f32_max_samples(1, 128) and det.samples_seen == 0
    assert det.state.shape == (2, lib.ofs_aa_chunk_f32_state_bytes(1, 128)) and not bool(det.state.any())
    with pytest.raises(ValueError, match="complex64"):
        det.push(torch.zeros((2, 1, 64, 2), dtype=torch.int16))
    with pytest.raises(ValueError, match="complex64"):
        det.push(torch.zeros((2, 1, 64), dtype=torch.complex128))
    with pytest.raises(ValueError, match=r"\[2, 1, Tc\] complex64"):
        det.push(torch.zeros((3, 1, 64), dtype=torch.complex64))
    with pytest.raises(ValueError, match="final=True"):
        det.push(torch.zeros((2, 0), dtype=torch.complex64))
    two = sync_aa.AAChunkedDetectorF32(2, 2, 256, device="cpu")
    with pytest.raises(ValueError, match=r"\[2, 2, Tc\] complex64"):
        two.push(torch.zeros((2, 64), dtype=torch.complex64))         # [B, Tc] is for one antenna
    for bad in ({"L": 64}, {"L": 2048}, {"n_ant": 3}):
        with pytest.raises(ValueError, match="128/256/512/1024"):
            sync_aa.AAChunkedDetectorF32(1, **{"n_ant": 1, "L": 128, **bad}, device="cpu")
    assert det.samples_seen == 0
