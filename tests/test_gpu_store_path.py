"""GPU: the store path of the one-antenna register-staged [A][A] kernel (aa_fast.hip: row-paired
16-byte R/M stores, variant FAST_RMPAIR; output store cache policy, variant FAST_ST_POLICY).

Only the stores move, so every arm must give the SAME bits as the arm with pairing off and plain
stores, must match the fp64 C oracle like the headline does, and must write nothing outside its
output arrays.  The kernel is called through the C ABI (ofs_aa_detect) so that the test owns the
output buffers: each output is a view into a larger allocation with a guard band of sentinel
bytes on both sides.

B = 5: odd stream indices make b*T only 8-byte aligned for R and M when T % 4 == 2.
L = 128, 256, 512 are windows of 1, 2, 4 rows (two samples per lane).  Stream lengths:
1024 all rows paired; 1022 T % 4 = 2, every row falls back; 640 five rows, the last unpaired;
516 row 4 partial, row 5 absent; 256 exactly one pair; 128 a single row; 4, 2 tiny streams
(T < L included).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 5
E = 4                                   # max_events
LS = (128, 256, 512)
TS = (1024, 1022, 640, 516, 256, 128, 4, 2)
SUBSETS = (("P", "R", "M"), ("R",), ("M",), ("P", "M"), ("P", "R", "M", "valid"))
# (FAST_RMPAIR, FAST_ST_POLICY) arms of the committed kernel; the first is the reference arm
ARMS = ((0, 0), (1, 0), (0, 1), (1, 1))
GUARD = 2048                            # sentinel bytes on each side of every output (>= 1 KiB, 16-byte multiple)
SENTINEL = 0xA5
DTYPES = {"P": torch.complex64, "R": torch.float32, "M": torch.float32, "valid": torch.uint8}


@functools.lru_cache(maxsize=None)
def stream_batch(T, L):
    """[B, 1, T] complex64 (host): noise, and from T/4 on a period-L signal under it (the window
    metric rises to ~1 one period later, so the longer streams hold gates, peaks and CFO events)."""
    rng = np.random.default_rng(1000 * L + T)
    x = 0.25 * (rng.standard_normal((B, T)) + 1j * rng.standard_normal((B, T)))
    for b in range(B):
        a = rng.standard_normal(L) + 1j * rng.standard_normal(L)
        n = np.arange(T)
        sig = a[n % L] * np.exp(2j * np.pi * 0.0003 * (b + 1) * n)
        x[b] += np.where(n >= T // 4 + 3 * b, sig, 0)
    return np.ascontiguousarray(x[:, None, :].astype(np.complex64))


@functools.lru_cache(maxsize=None)
def oracle(T, L):
    import oracle_c
    return oracle_c.aa_detect(stream_batch(T, L), L, max_events=E, nthreads=4)


class Guarded:
    """An output array as a view into a larger allocation, sentinel bytes on both sides."""

    def __init__(self, dtype, dev):
        self.nbytes = B * 1024 * 8 + 2 * GUARD          # room for the largest output (c64, T = 1024)
        self.raw = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.dtype = dtype

    def view(self, T):
        self.raw.fill_(SENTINEL)
        self.n = B * T * torch.empty((), dtype=self.dtype).element_size()
        return self.raw[GUARD:GUARD + self.n].view(self.dtype).view(B, T)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == SENTINEL).all()) and bool((self.raw[GUARD + self.n:] == SENTINEL).all())


@pytest.fixture(scope="module")
def bufs():
    dev = torch.device("cuda", 0)
    return dev, {k: Guarded(dt, dev) for k, dt in DTYPES.items()}


def run_arm(bufs, T, L, subset, arm):
    """One ofs_aa_detect call into guarded buffers under the arm's variants (None: default
    dispatch); returns the outputs, the events and whether every guard band is untouched."""
    from ofdm_sync_amd import _lib
    dev, g = bufs
    x = torch.from_numpy(stream_batch(T, L)).to(dev)
    out = {k: g[k].view(T) for k in subset}
    n_ev = torch.zeros(B, dtype=torch.int32, device=dev)
    ev_i = torch.zeros((B, E, 4), dtype=torch.int64, device=dev)
    ev_r = torch.zeros((B, E, 4), dtype=torch.float64, device=dev)
    ptr = lambda k: out[k].data_ptr() if k in out else None  # noqa: E731
    kw = {} if arm is None else dict(FAST_RMPAIR=arm[0], FAST_ST_POLICY=arm[1])
    with _lib.variants(**kw):
        rc = _lib.lib().ofs_aa_detect(_lib.C64, x.data_ptr(), B, 1, T, L, _lib.FP32, ptr("P"), ptr("R"), ptr("M"),
                                      ptr("valid"), 1, 0.15, 128, 15.36e6, E, n_ev.data_ptr(), ev_i.data_ptr(),
                                      ev_r.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    res = {k: v.clone() for k, v in out.items()}
    res.update(n_events=n_ev, ev_int=ev_i, ev_real=ev_r)
    return res, all(g[k].guards_intact() for k in subset)


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("T", TS)
def test_arms_bit_identical_and_no_stray_bytes(bufs, T, L):
    from ofdm_sync_amd import _lib
    assert _lib.lib().ofs_aa_plan(_lib.C64, _lib.FP32, 1, T, L) == 1020 + L // 128     # register-staged, E = 2
    for subset in SUBSETS:
        ref, intact = run_arm(bufs, T, L, subset, ARMS[0])
        assert intact, (subset, ARMS[0])
        for arm in ARMS[1:] + (None,):
            got, intact = run_arm(bufs, T, L, subset, arm)
            assert intact, (subset, arm)
            for k in ref:
                a, b = ref[k], got[k]
                if a.is_complex():
                    a, b = torch.view_as_real(a), torch.view_as_real(b)
                if a.is_floating_point():                    # bits, not values (NaN-safe, signed zeros)
                    a, b = a.view(torch.int32 if a.element_size() == 4 else torch.int64), b.view(
                        torch.int32 if b.element_size() == 4 else torch.int64)
                assert torch.equal(a, b), (subset, arm, k)


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("T", TS)
def test_default_arm_matches_oracle(bufs, T, L):
    import parity
    o = oracle(T, L)
    got, intact = run_arm(bufs, T, L, ("P", "R", "M"), None)
    assert intact
    r = parity.classify_aa(got["M"].cpu().numpy().astype(np.float64), got["n_events"].cpu().numpy(),
                           got["ev_int"].cpu().numpy(), got["ev_real"].cpu().numpy(), o["P"], o["M"],
                           o["n_events"], o["ev_int"], o["ev_real"], L)
    print("store path parity", T, L, r)
    assert r["mismatch"] == 0, r
    assert r["cfo_over_tol"] == 0, r
    assert r["max_abs_err_M"] <= 1e-6, r
    if T >= 4 * L:
        assert int(o["n_events"].sum()) > 0                  # the long streams do hold events
