"""CPU: ofs_zc_detect_chunk / ofs_zc_chunk_state_bytes are declared, exported and refuse every bad
argument the header lists before any launch (no GPU here: small integers stand in for device pointers,
so a call that got past the checks would fault or return a HIP error instead of OFS_EINVAL)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ofdmsync.h")
LIB = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
EINVAL = -1
MAX_W, MAX_H = 1 << 16, 1 << 28


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build_hip()
    l = ctypes.CDLL(LIB)
    from ofdm_sync_amd import _lib as L
    L._declare(l)
    return l


def test_declared_and_exported(lib):
    txt = open(HEADER).read()
    for s in ("ofs_zc_chunk_state_bytes", "ofs_zc_detect_chunk"):
        assert re.search(r"^\s*int(32|64)_t\s+" + s + r"\s*\(", txt, re.M), s
        assert hasattr(lib, s), s
    out = os.popen(f"nm -D --defined-only {LIB}").read()
    assert re.search(r"\bT\s+ofs_zc_detect_chunk$", out, re.M) and re.search(r"\bT\s+ofs_zc_chunk_state_bytes$", out, re.M)
    assert re.search(r"#define\s+OFS_ZC_CHUNK_MAX_WINDOW\s+\(1 << 16\)", txt)
    assert re.search(r"#define\s+OFS_ZC_CHUNK_MAX_HYSTERESIS\s+\(1 << 28\)", txt)
    # the chunk entry's comment carries the guarantee, like the two other chunk entries
    at = txt.index("Resumable chunked zc_v2")
    assert "EQUIVALENCE GUARANTEE" in txt[at:txt.index("int32_t ofs_zc_detect_chunk(")]


def test_python_binding_declares_both(lib):
    from ofdm_sync_amd import _lib as L
    import inspect
    src = inspect.getsource(L._declare)
    assert '"ofs_zc_chunk_state_bytes"' in src and '"ofs_zc_detect_chunk"' in src
    assert len(lib.ofs_zc_detect_chunk.argtypes) == 24


def test_state_bytes(lib):
    f = lib.ofs_zc_chunk_state_bytes
    for W in (1, 100, 128, 2048, 65536):
        n = f(W)
        assert n > 0 and n % 16 == 0 and n >= 8 * W + 16, (W, n)
    assert f(0) == f(1)                                    # RunningSum: max(1, W)
    assert f(MAX_W + 1) == EINVAL and f(-1) == EINVAL and f(-(1 << 31)) == EINVAL
    assert f(MAX_W) > f(2048) > f(128)


# a valid call in keyword form; every refusal below changes one argument of it
GOOD = dict(corr_mag=64, ld_mag=256, B=4, Tc=256, window_size=128, thresh_value=1, thresh_frac_bits=15,
            min_corr_mag=0.5, reference_length=100, hysteresis=256, state=1024, local_sum=None,
            corr_scaled=None, thresh_scaled=None, above_threshold=None, metric_valid=None, gate_mask=None,
            max_events=4, n_events=64, ev_int=64, ev_peak=64, open_gate_start=64, final=0, stream=None)


def call(lib, **kw):
    a = dict(GOOD, **kw)
    assert list(a) == list(GOOD)
    return lib.ofs_zc_detect_chunk(*a.values())


@pytest.mark.parametrize("kw", [
    dict(B=-1), dict(Tc=-1),
    dict(Tc=0, final=0),                                   # an empty chunk is a flush only
    dict(ld_mag=255), dict(ld_mag=0),                      # rows overlap (B > 1)
    dict(window_size=MAX_W + 1),
    dict(thresh_frac_bits=-1), dict(thresh_frac_bits=63),
    dict(hysteresis=-1), dict(hysteresis=MAX_H + 1),
    dict(max_events=-1),
    dict(state=None), dict(state=1032),                    # null / not 16-byte aligned
    dict(corr_mag=None), dict(corr_mag=68),                # null with samples / not 8-byte aligned
    dict(n_events=None), dict(open_gate_start=None),
    dict(ev_int=None), dict(ev_peak=None),                 # max_events > 0
    dict(B=1, ld_mag=0, state=None),                       # one stream: ld_mag is free, the state is not
], ids=str)
def test_refused_before_any_launch(lib, kw):
    assert call(lib, **kw) == EINVAL


def test_empty_batch_is_a_noop_with_null_pointers(lib):
    assert call(lib, B=0, corr_mag=None, state=None, n_events=None, ev_int=None, ev_peak=None,
                open_gate_start=None) == 0
    assert call(lib, B=0, Tc=0, final=1, ld_mag=0, corr_mag=None, state=None, n_events=None, ev_int=None,
                ev_peak=None, open_gate_start=None) == 0
    # ... but its scalar arguments are still checked
    assert call(lib, B=0, thresh_frac_bits=70, corr_mag=None, state=None, n_events=None, ev_int=None,
                ev_peak=None, open_gate_start=None) == EINVAL
