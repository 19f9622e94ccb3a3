"""CPU: the scaffolding the seven resumable chunked classes share (ofdm_sync_amd/_chunked.py), on every
one of them: construction, the chunk each expects (a ValueError that names it, raised before anything is
allocated or launched), and reset.  ``device="cpu"``: no launch happens here."""
import ctypes
import os

import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

LIB = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
B = 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build_hip()
    from ofdm_sync_amd import _lib as L
    l = ctypes.CDLL(LIB)
    L._declare(l)
    return l


def _z(shape, dtype):
    return torch.zeros(shape, dtype=dtype)


def _cases():
    """name -> (constructor, size-function prefix, their arguments, a chunk of Tc samples for B streams,
    [(bad chunk, text the ValueError must hold)]).  Every class: a wrong dtype, a wrong B, a wrong branch
    count (where a chunk has a branch axis) and an empty non-final chunk."""
    from ofdm_sync_amd import _lib, _metrics, minn_rtl, park, sync_aa, zc_freq, zc_v2
    c64, c128, i16, u8, f64 = torch.complex64, torch.complex128, torch.int16, torch.uint8, torch.float64
    return {
        "aa_int16": (lambda: sync_aa.AAChunkedDetector(B, 1, 128, device="cpu"), "ofs_aa_chunk", (1, 128),
                     lambda b, Tc: _z((b, 1, Tc, 2), i16),
                     [(_z((B, 1, 64), c64), r"\[2, 1, Tc, 2\] int16"), (_z((3, 1, 64, 2), i16), r"\[2, 1, Tc, 2\] int16"),
                      (_z((B, 2, 64, 2), i16), r"\[2, 1, Tc, 2\] int16"), (_z((B, 1, 0, 2), i16), "final=True")]),
        "aa_cp12": (lambda: sync_aa.AAChunkedDetector(B, 2, 256, in_dtype="cp12", device="cpu"), "ofs_aa_chunk",
                    (2, 256), lambda b, Tc: _z((b, Tc, 6), u8),
                    [(_z((B, 2, 64, 2), i16), r"\[2, Tc, 6\] uint8"), (_z((3, 64, 6), u8), r"\[2, Tc, 6\] uint8"),
                     (_z((B, 64, 3), u8), r"\[2, Tc, 6\] uint8"), (_z((B, 0, 6), u8), "final=True")]),
        "aa_f32": (lambda: sync_aa.AAChunkedDetectorF32(B, 1, 128, device="cpu"), "ofs_aa_chunk_f32", (1, 128),
                   lambda b, Tc: _z((b, 1, Tc), c64),
                   [(_z((B, 1, 64), c128), "complex64"), (_z((3, 1, 64), c64), r"\[2, 1, Tc\] complex64"),
                    (_z((B, 2, 64), c64), r"\[2, 1, Tc\] complex64"), (_z((B, 0), c64), "final=True")]),
        "rtl": (lambda: minn_rtl.MinnRTLChunkedDetector(B, 64, 2, device="cpu"), "ofs_rtl_chunk", (2, 64),
                lambda b, Tc: _z((b, 2, Tc, 2), i16),
                [(_z((B, 2, 64, 2), torch.int32), r"\[2, 2, Tc, 2\] int16"), (_z((1, 2, 64, 2), i16), r"\[2, 2, Tc, 2\] int16"),
                 (_z((B, 1, 64, 2), i16), r"\[2, 2, Tc, 2\] int16"), (_z((B, 2, 0, 2), i16), "final=True")]),
        "win": (lambda: _metrics.WindowMetricChunked("minn", B, 2, 512, device="cpu"), "ofs_win_chunk", (3, 2, 512),
                lambda b, Tc: _z((b, 2, Tc), c64),
                [(_z((B, 2, 64, 2), i16), "complex64"), (_z((3, 2, 64), c64), r"\[2, 2, Tc\] complex64"),
                 (_z((B, 64), c64), r"\[2, 2, Tc\] complex64"), (_z((B, 2, 0), c64), "final=True")]),
        "park": (lambda: park.ParkChunkedMetric(B, 1, 8, dtype=i16, device="cpu"), "ofs_park_chunk", (_lib.CI16, 1, 8),
                 lambda b, Tc: _z((b, 1, Tc, 2), i16),
                 [(_z((B, 1, 64), c64), r"\[2, 1, Tc, 2\] torch.int16"), (_z((3, 1, 64, 2), i16), r"\[2, 1, Tc, 2\] torch.int16"),
                  (_z((B, 2, 64, 2), i16), r"\(or \[2, Tc, 2\]\)"), (_z((B, 0, 2), i16), "final=True")]),
        "zc_freq": (lambda: zc_freq.FrequencyMetricChunked(B, 2, dtype=c128, N=64, cp=5, device="cpu"),
                    "ofs_zc_freq_chunk", (_lib.C128, 2, 64, 5), lambda b, Tc: _z((b, 2, Tc), c128),
                    [(_z((B, 2, 64), c64), r"\[2, 2, Tc\] torch.complex128"), (_z((3, 2, 64), c128), r"\[2, 2, Tc\] torch.complex128"),
                     (_z((B, 64), c128), r"\[2, 2, Tc\] torch.complex128"), (_z((B, 2, 0), c128), "final=True")]),
        # magnitudes have no branch axis
        "zc": (lambda: zc_v2.ZCChunkedDetector(B, [1.0, 1j, -1.0], window_size=32, device="cpu"), "ofs_zc_chunk", (32,),
               lambda b, Tc: _z((b, Tc), f64),
               [(_z((B, 64), torch.float32), r"\[2, Tc\] float64"), (_z((3, 64), f64), r"\[2, Tc\] float64"),
                (_z((B, 1, 64), f64), r"\[2, Tc\] float64"), (_z((B, 0), f64), "final=True")]),
    }


NAMES = ("aa_int16", "aa_cp12", "aa_f32", "rtl", "win", "park", "zc_freq", "zc")


def _push(det, x):
    return det.push_mag(x) if hasattr(det, "push_mag") else det.push(x)


@pytest.mark.parametrize("name", NAMES)
def test_construction_bad_chunks_and_reset(lib, name):
    from ofdm_sync_amd import _chunked
    make, sizes, args, chunk, bad = _cases()[name]
    det = make()
    assert isinstance(det, _chunked.ChunkedStreams) and det.B == B and det.device == torch.device("cpu")
    nbytes = getattr(lib, sizes + "_state_bytes")(*args)
    assert nbytes > 0 and nbytes % 16 == 0
    assert det.state.shape == (B, nbytes) and det.state.dtype == torch.uint8 and not bool(det.state.any())
    if name == "zc":
        assert det.max_chunk is None                                   # ofs_zc_detect_chunk has no limit
    else:
        assert det.max_chunk == getattr(lib, sizes + "_max_samples")(*args) > 0
    assert det.samples_seen == 0
    if name == "zc_freq":
        assert det.n_seen == 0

    for x, text in bad:
        with pytest.raises(ValueError, match=text):
            _push(det, x)
    if det.max_chunk is not None:
        shape = list(chunk(B, 1).shape)
        t_axis = [i for i, (a, b) in enumerate(zip(shape, chunk(B, 2).shape)) if a != b][0]
        shape[t_axis] = det.max_chunk + 1
        big = torch.zeros((), dtype=chunk(B, 1).dtype).expand(*shape)  # no storage behind it
        with pytest.raises(ValueError, match=f"max_chunk = {det.max_chunk}"):
            _push(det, big)
    # nothing was counted, allocated or written
    assert det.samples_seen == 0 and not det._bufs and not bool(det.state.any())
    if name == "zc_freq":
        assert det._buf is None
    if name == "zc":
        assert det.history is None

    det.state.fill_(1)
    det.samples_seen = 7
    det.reset(torch.tensor([False, True]))
    assert bool((det.state[0] == 1).all()) and not bool(det.state[1].any())
    assert det.samples_seen == 7                                       # restarts only on a full reset
    det.state.fill_(1)
    det.reset([True, False])                                           # anything torch.as_tensor takes
    assert not bool(det.state[0].any()) and bool((det.state[1] == 1).all())
    det.reset()
    assert not bool(det.state.any()) and det.samples_seen == 0


def test_frequency_metric_resets_rows_by_index(lib):
    """``FrequencyMetricChunked.reset`` also takes stream indices; ``n_seen`` is the base's counter."""
    det = _cases()["zc_freq"][0]()
    det.state.fill_(1)
    det.n_seen = 5
    assert det.samples_seen == 5
    det.reset([1])
    assert bool((det.state[0] == 1).all()) and not bool(det.state[1].any()) and det.n_seen == 5
    det.reset()
    assert not bool(det.state.any()) and det.n_seen == 0 and det.samples_seen == 0
