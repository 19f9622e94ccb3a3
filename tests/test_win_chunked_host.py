"""CPU: the chunked window-metric entry points (include/ofdmsync.h, ofs_win_metric_chunk) size their
state and reject bad arguments before any GPU call, and WindowMetricChunked names the chunk it expects.
No launch happens here."""
import ctypes
import os

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
EINVAL = -1
C64, FP32 = 0, 0
MAX_TC = 1 << 30                       # the documented ofs_win_chunk_max_samples
WINDOWS = (128, 256, 512, 1024, 2048)
NAMES = ("ofs_win_chunk_state_bytes", "ofs_win_chunk_max_samples", "ofs_win_metric_chunk")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build_hip()
    from ofdm_sync_amd import _lib as L
    l = ctypes.CDLL(LIB)
    L._declare(l)
    return l


def _supported(kind, n_br, N):
    """The header's table, written out: window N/2 (kinds 1, 2) or N/4 (kind 3) in WINDOWS, 1-2 branches,
    2048 with one branch only."""
    if kind not in (1, 2, 3) or n_br not in (1, 2):
        return False
    div = 4 if kind == 3 else 2
    if N <= 0 or N % div:
        return False
    W = N // div
    return W in WINDOWS and not (n_br == 2 and W == 2048)


def test_symbols_exported_and_declared(lib):
    src = open(os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "_lib.py")).read()
    hdr = open(os.path.join(ROOT, "include", "ofdmsync.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert f'"{name}"' in src and f"{name}(" in hdr, name
    assert len(lib.ofs_win_metric_chunk.argtypes) == 13
    assert len(lib.ofs_win_chunk_state_bytes.argtypes) == 3 and len(lib.ofs_win_chunk_max_samples.argtypes) == 3
    at = hdr.index("Resumable chunked S&C")
    assert "EQUIVALENCE GUARANTEE" in hdr[at:hdr.index("int32_t ofs_win_metric_chunk(")]


def test_shape_tables_follow_the_one_shot_plan(lib):
    """state_bytes > 0 exactly where the one-shot call has a fast plan (kinds 1-3); there it is a
    multiple of 16, does not shrink with a second branch, holds the history, and max_samples is the
    documented 2^30.  Both helpers are < 0 everywhere else (kind 4 included)."""
    lens = sorted(set(range(0, 8193, 64)) | {258, 1023})
    n_ok = 0
    for kind in (1, 2, 3, 4):
        for N in lens:
            one = None
            for n_br in (1, 2, 3):
                plan = lib.ofs_win_plan(kind, C64, FP32, n_br, N, N)
                sb = lib.ofs_win_chunk_state_bytes(kind, n_br, N)
                cap = lib.ofs_win_chunk_max_samples(kind, n_br, N)
                ok = plan > 0 and kind <= 3
                assert ok == _supported(kind, n_br, N), (kind, n_br, N, plan)
                assert (sb > 0) == ok, (kind, n_br, N, plan, sb)
                if not ok:
                    assert sb < 0 and cap < 0, (kind, n_br, N, sb, cap)
                    continue
                n_ok += 1
                assert sb % 16 == 0 and cap == MAX_TC, (kind, n_br, N, sb, cap)
                E, MW = plan // 10, plan % 10
                hist = ((0, MW, 2 * MW)[kind - 1] + 2 * MW) * 64 * E + 64 * E - 1      # rows + n_seen % RL
                assert sb >= n_br * hist * 8, (kind, n_br, N, sb)
                assert hist <= 1.5 * N + 64 * E
                if n_br == 1:
                    one = sb
                else:
                    assert one is not None and sb >= one, (kind, N, one, sb)
    assert n_ok == 3 * (5 + 4)
    for kind in (0, -1, 5):
        assert lib.ofs_win_chunk_state_bytes(kind, 1, 2048) < 0 and lib.ofs_win_chunk_max_samples(kind, 1, 2048) < 0
    assert lib.ofs_win_chunk_state_bytes(1, 1, -2048) < 0 and lib.ofs_win_chunk_state_bytes(1, 0, 2048) < 0


def test_in_call_positions_fit_32_bits(lib):
    """history (at most 1.5 N + 255) + chunk + one row of padding < 2^31 at the largest N."""
    assert 3 * 8192 // 2 + 255 + MAX_TC + 256 < 1 << 31


def _call(lib, kind=2, x=16, B=1, n_br=1, Tc=256, N=2048, state=16, final=0):
    """ofs_win_metric_chunk with small non-null integers standing in for device pointers: every case
    below must be refused before anything is dereferenced or launched."""
    return lib.ofs_win_metric_chunk(kind, x, B, n_br, Tc, N, state, None, None, None, None, final, None)


def test_argument_validation_without_gpu(lib):
    """Each case of the header's OFS_EINVAL list returns it (before any HIP call)."""
    for kind in (0, 4, 5, -1):
        assert _call(lib, kind=kind) == EINVAL
    for n_br in (0, 3):
        assert _call(lib, n_br=n_br) == EINVAL
    for N in (0, 64, 128, 258, 1023, 2048 + 64, 3072, 8192, -2048):
        assert _call(lib, kind=1, N=N) == EINVAL, N
    assert _call(lib, kind=3, N=256) == EINVAL                         # Minn window 64: below one row
    assert _call(lib, kind=3, N=8192, n_br=2) == EINVAL                # W = 2048 with two branches
    assert _call(lib, kind=2, N=4096, n_br=2) == EINVAL
    for kind, n_br, N in ((1, 1, 256), (2, 2, 2048), (3, 1, 8192), (3, 2, 4096)):
        cap = lib.ofs_win_chunk_max_samples(kind, n_br, N)
        assert cap > 0
        assert _call(lib, kind=kind, n_br=n_br, N=N, Tc=cap + 1) == EINVAL
    assert _call(lib, Tc=0, final=0) == EINVAL                         # empty chunk that is no flush
    assert _call(lib, Tc=-1, final=1) == EINVAL
    assert _call(lib, B=-1) == EINVAL
    assert _call(lib, state=None) == EINVAL                            # null state with B > 0
    assert _call(lib, state=None, Tc=0, final=1) == EINVAL             # ... also for a flush
    assert _call(lib, state=8) == EINVAL                               # state not 16-byte aligned
    assert _call(lib, x=None) == EINVAL                                # null samples with B * Tc > 0


def test_empty_batch_is_a_valid_no_op(lib):
    """B = 0 launches nothing and every pointer may be null."""
    for kind in (1, 2, 3):
        assert _call(lib, kind=kind, B=0, x=None, state=None) == 0
        assert _call(lib, kind=kind, B=0, x=None, state=None, Tc=0, final=1) == 0
    assert _call(lib, kind=4, B=0, x=None, state=None) == EINVAL       # the shape is checked first


def test_python_names_the_expected_chunk(lib):
    """Wrong dtype or shape: a ValueError that says what a chunk looks like (raised before any launch)."""
    torch = pytest.importorskip("torch")
    from ofdm_sync_amd import _metrics, combined_sc_min, minn, sc
    det = _metrics.WindowMetricChunked("comb", 2, 1, 256, device="cpu")
    assert det.kind == 2 and det.max_chunk == MAX_TC and det.samples_seen == 0
    assert det.state.shape == (2, lib.ofs_win_chunk_state_bytes(2, 1, 256)) and not bool(det.state.any())
    assert det.state.dtype == torch.uint8
    with pytest.raises(ValueError, match="complex64"):
        det.push(torch.zeros((2, 1, 64, 2), dtype=torch.int16))
    with pytest.raises(ValueError, match="complex64"):
        det.push(torch.zeros((2, 1, 64), dtype=torch.complex128))
    with pytest.raises(ValueError, match=r"\[2, 1, Tc\] complex64"):
        det.push(torch.zeros((3, 1, 64), dtype=torch.complex64))
    with pytest.raises(ValueError, match="final=True"):
        det.push(torch.zeros((2, 0), dtype=torch.complex64))
    big = torch.zeros((), dtype=torch.complex64).expand(2, 1, MAX_TC + 1)     # no storage behind it
    with pytest.raises(ValueError, match="max_chunk"):
        det.push(big)
    two = _metrics.WindowMetricChunked(3, 2, 2, 512, device="cpu")
    assert two.kind == 3
    with pytest.raises(ValueError, match=r"\[2, 2, Tc\] complex64"):
        two.push(torch.zeros((2, 64), dtype=torch.complex64))         # [B, Tc] is for one branch
    for bad in ({"symbol_len": 128}, {"symbol_len": 3072}, {"n_branch": 3}, {"symbol_len": 4096, "n_branch": 2}):
        with pytest.raises(ValueError, match="128/256/512/1024/2048"):
            _metrics.WindowMetricChunked("sc", 1, **{"n_branch": 1, "symbol_len": 256, **bad}, device="cpu")
    with pytest.raises(ValueError, match="kind"):
        _metrics.WindowMetricChunked(4, 1, 1, 2048, device="cpu")
    with pytest.raises(ValueError, match="outputs"):
        _metrics.WindowMetricChunked("sc", 1, 1, 2048, outputs=("M", "valid"), device="cpu")
    assert det.samples_seen == 0 and not det._bufs
    # the reference's module names: kind and symbol length (N_FFT read at construction)
    a = sc.SCChunkedMetric(3, device="cpu")
    assert (a.kind, a.symbol_len, a.B, a.n_branch) == (1, sc.N_FFT, 3, 1)
    old, sc.N_FFT = sc.N_FFT, 512
    try:
        assert sc.SCChunkedMetric(1, 2, device="cpu").symbol_len == 512
    finally:
        sc.N_FFT = old
    assert combined_sc_min.SCChunkedMetric(1, device="cpu").kind == 2
    assert minn.MinnChunkedMetric(1, 1, 1024, device="cpu").kind == 3
    assert combined_sc_min.MinnChunkedMetric(1, device="cpu").symbol_len == combined_sc_min.N_FFT
    both = combined_sc_min.SCMinnChunkedMetrics(2, 1, 1024, outputs=("M",), device="cpu")
    assert (both.minn.kind, both.sc.kind, both.max_chunk, both.samples_seen) == (3, 2, MAX_TC, 0)
    with pytest.raises(ValueError, match="final=True"):
        both.push(torch.zeros((2, 0), dtype=torch.complex64))
