"""GPU: the input load path of the full-stream form of the register-staged [A][A] kernel (aa_fast.hip,
template parameter LP, variant FAST_LD_POLICY).

Only the cache policy of the loads of x changes between the arms (0 plain, 1 non-temporal: the default),
so every arm must give the SAME bits as LP 0 in P, R, M, n_events and the event arrays, and the default
dispatch must match the fp64 C oracle as test_gpu_store_path's default arm does.  The kernel is called
through the C ABI (ofs_aa_detect_ex) on the full-stream shape: one antenna, T = 1024, P, R, M and the
events.  B = 5 streams; L = 128, 256, 512 are windows of 1, 2, 4 rows; hysteresis 128 runs the scan-free
gate rows and 16 the scan rows; the resident-head flag is passed on and off (the heads hold zeros, as the
flag promises).  One case reads x through a view offset by one sample, so that every stream's base is
only 8-byte aligned.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 5
T = 1024
E = 4                                   # max_events
LS = (128, 256, 512)
HYSTS = (128, 16)
HEAD_FLAG = 1                           # OFS_AA_HEAD_RESIDENT
# FAST_LD_POLICY arms of the committed kernel besides the reference arm 0
ARMS = (1,)


@functools.lru_cache(maxsize=None)
def stream_batch(L):
    """[B, 1, T] complex64 (host): noise, and from T/4 on a period-L signal under it (as
    test_gpu_store_path.stream_batch)."""
    rng = np.random.default_rng(1000 * L + T)
    x = 0.25 * (rng.standard_normal((B, T)) + 1j * rng.standard_normal((B, T)))
    for b in range(B):
        a = rng.standard_normal(L) + 1j * rng.standard_normal(L)
        n = np.arange(T)
        sig = a[n % L] * np.exp(2j * np.pi * 0.0003 * (b + 1) * n)
        x[b] += np.where(n >= T // 4 + 3 * b, sig, 0)
    return np.ascontiguousarray(x[:, None, :].astype(np.complex64))


@functools.lru_cache(maxsize=None)
def oracle(L):
    import oracle_c
    return oracle_c.aa_detect(stream_batch(L), L, max_events=E, nthreads=4)


@functools.lru_cache(maxsize=None)
def device_x(L, offset):
    """x on the device; offset = 1: a view one sample into a larger allocation (8-byte-aligned base)."""
    dev = torch.device("cuda", 0)
    raw = torch.zeros(B * T + offset, dtype=torch.complex64, device=dev)
    x = raw[offset:].view(B, 1, T)
    x.copy_(torch.from_numpy(stream_batch(L)))
    assert x.data_ptr() % 16 == (8 if offset else 0)
    return x


def bits(t):
    """Integer view of a tensor (bit comparison: NaN-safe, signed zeros told apart)."""
    if t.is_complex():
        t = torch.view_as_real(t)
    if t.is_floating_point():
        t = t.view(torch.int32 if t.element_size() == 4 else torch.int64)
    return t


def run_arm(x, L, lp, hyst=128, flags=0):
    """One ofs_aa_detect_ex call under FAST_LD_POLICY = lp (None: default dispatch) into zeroed outputs."""
    from ofdm_sync_amd import _lib
    dev = x.device
    out = {"P": torch.zeros((B, T), dtype=torch.complex64, device=dev),
           "R": torch.zeros((B, T), dtype=torch.float32, device=dev),
           "M": torch.zeros((B, T), dtype=torch.float32, device=dev),
           "n_events": torch.zeros(B, dtype=torch.int32, device=dev),
           "ev_int": torch.zeros((B, E, 4), dtype=torch.int64, device=dev),
           "ev_real": torch.zeros((B, E, 4), dtype=torch.float64, device=dev)}
    with _lib.variants(**({} if lp is None else {"FAST_LD_POLICY": lp})):
        rc = _lib.lib().ofs_aa_detect_ex(_lib.C64, x.data_ptr(), B, 1, T, L, _lib.FP32, out["P"].data_ptr(),
                                         out["R"].data_ptr(), out["M"].data_ptr(), None, 1, 0.15, hyst, 15.36e6, E,
                                         out["n_events"].data_ptr(), out["ev_int"].data_ptr(),
                                         out["ev_real"].data_ptr(), torch.cuda.current_stream().cuda_stream, flags)
    assert rc == 0
    torch.cuda.synchronize()
    return out


def assert_arms_equal(x, L, hyst, flags):
    ref = run_arm(x, L, 0, hyst, flags)
    assert int(ref["n_events"].sum()) > 0                        # the streams do hold events
    for lp in ARMS + (None, 99):                                 # 99: an unknown value is the default arm
        got = run_arm(x, L, lp, hyst, flags)
        for k in ref:
            assert torch.equal(bits(ref[k]), bits(got[k])), (lp, hyst, flags, k)
    return ref


@pytest.mark.parametrize("flags", (0, HEAD_FLAG))
@pytest.mark.parametrize("hyst", HYSTS)
@pytest.mark.parametrize("L", LS)
def test_arms_bit_identical(L, hyst, flags):
    from ofdm_sync_amd import _lib
    assert _lib.lib().ofs_aa_plan(_lib.C64, _lib.FP32, 1, T, L) == 1020 + L // 128     # register-staged, E = 2
    assert_arms_equal(device_x(L, 0), L, hyst, flags)


@pytest.mark.parametrize("L", LS)
def test_offset_view_behaves_as_plain_loads(L):
    """x one sample into its allocation: every arm, and the default, give what LP 0 gives there - which
    is what LP 0 gives on the aligned copy of the same samples."""
    for hyst in HYSTS:
        off = assert_arms_equal(device_x(L, 1), L, hyst, 0)
        aligned = run_arm(device_x(L, 0), L, 0, hyst, 0)
        for k in off:
            assert torch.equal(bits(off[k]), bits(aligned[k])), (hyst, k)


@pytest.mark.parametrize("L", LS)
def test_default_arm_matches_oracle(L):
    import parity
    o = oracle(L)
    got = run_arm(device_x(L, 0), L, None)
    r = parity.classify_aa(got["M"].cpu().numpy().astype(np.float64), got["n_events"].cpu().numpy(),
                           got["ev_int"].cpu().numpy(), got["ev_real"].cpu().numpy(), o["P"], o["M"],
                           o["n_events"], o["ev_int"], o["ev_real"], L)
    print("load path parity", L, r)
    assert r["mismatch"] == 0, r
    assert r["cfo_over_tol"] == 0, r
    assert r["max_abs_err_M"] <= 1e-6, r
    if T >= 4 * L:
        assert int(o["n_events"].sum()) > 0                      # the long streams do hold events
