"""GPU: the full-stream form of the register-staged [A][A] kernel (aa_fast.hip, template flag FS;
variant FAST_FULL = 0 sends the same call to the generic form).

The full-stream form runs when one antenna, T = 1024, L = 128 | 256 | 512, P, R and M, no valid and
the events are all asked for.  It only drops generality (stream length, pointer tests, per-row address
arithmetic, the per-row choice of gate machine, the fp64 threshold compare), so every output must be
the generic form's bit for bit, nothing may be written outside the output arrays, and every call the
specialised form does not cover must be unaffected by the variant.  The kernels are called through the
C ABI (ofs_aa_detect / ofs_aa_detect_ex) so that the test owns the buffers: each output is a view into
a larger allocation with 2 KiB of sentinel bytes on both sides, filled with the sentinel before a call.

Inputs: B streams of noise with a period-L signal under it from T/4 on (as test_gpu_store_path's
stream_batch).  In streams b % 4 == 1 the signal stops after 5L/2 samples and comes back 5L/4 later, so
at L = 128 they hold two gates even with a hysteresis of 128.  In streams b % 4 == 3 the signal runs
from n = 0 and changes sign near 1.55 L: the lagged products add up until there and cancel after it, the
metric rises to ~0.3 and falls back under the threshold near 1.7 L, so at every L - 512 included - a gate
opens and closes inside the stream, by hysteresis and not at T.  One extra stream (the last of the
B + 1 a call gets) holds a NaN and an Inf sample.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 1024
BS = (5, 257)
LS = (128, 256, 512)
E = 4                                   # max_events
GUARD = 2048
SENTINEL = 0xA5
SENT32 = int(np.frombuffer(bytes([SENTINEL] * 4), dtype=np.int32)[0])
HEAD_FLAG = 1                           # OFS_AA_HEAD_RESIDENT
DTYPES = {"P": torch.complex64, "R": torch.float32, "M": torch.float32, "valid": torch.uint8}
ALL = ("P", "R", "M")


@functools.lru_cache(maxsize=None)
def batch(B, L):
    """[B + 1, 1, T] complex64 (host); the last stream holds a NaN and an Inf sample."""
    rng = np.random.default_rng(7000 * L + B)
    n = np.arange(T)
    x = 0.25 * (rng.standard_normal((B + 1, T)) + 1j * rng.standard_normal((B + 1, T)))
    for b in range(B + 1):
        a = rng.standard_normal(L) + 1j * rng.standard_normal(L)
        sig = a[n % L] * np.exp(2j * np.pi * 0.0003 * (b % 7 + 1) * n)
        s = T // 4 + 3 * (b % 16)
        on = n >= s
        if b % 4 == 1:
            on &= ~((n >= s + 5 * L // 2) & (n < s + 15 * L // 4))
        if b % 4 == 3:
            on = np.where(n >= (155 * L) // 100 + b % 16, -1, 1)
        x[b] += np.where(on, sig, 0) if b % 4 != 3 else on * sig
    x[B, 300] = complex(np.nan, 0.5)
    x[B, 700] = complex(np.inf, -1.0)
    return np.ascontiguousarray(x[:, None, :].astype(np.complex64))


class Guarded:
    """An output array as a view into a larger allocation, sentinel bytes on both sides."""

    def __init__(self, dtype, dev):
        self.raw = torch.empty((max(BS) + 1) * T * 8 + 2 * GUARD, dtype=torch.uint8, device=dev)
        self.dtype = dtype

    def view(self, nb, t):
        self.raw.fill_(SENTINEL)
        self.n = nb * t * torch.empty((), dtype=self.dtype).element_size()
        return self.raw[GUARD:GUARD + self.n].view(self.dtype).view(nb, t)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == SENTINEL).all()) and bool((self.raw[GUARD + self.n:] == SENTINEL).all())


@pytest.fixture(scope="module")
def bufs():
    dev = torch.device("cuda", 0)
    return dev, {k: Guarded(dt, dev) for k, dt in DTYPES.items()}


@functools.lru_cache(maxsize=None)
def device_batch(B, L, t=T):
    return torch.from_numpy(np.ascontiguousarray(batch(B, L)[:, :, :t])).to(torch.device("cuda", 0))


def bits(t):
    """Integer view of a tensor (bit comparison: NaN-safe, signed zeros told apart)."""
    if t.is_complex():
        t = torch.view_as_real(t)
    if t.is_floating_point():
        t = t.view(torch.int32 if t.element_size() == 4 else torch.int64)
    return t


def call(bufs, x, L, *, full, subset=ALL, flags=None, thr=0.15, hyst=128, max_ev=E, detect=1):
    """One call on the [nb, 1, t] device batch x into guarded, sentinel-filled buffers; full = None is
    the default dispatch, 0 the generic kernel (variant FAST_FULL).  Returns the outputs (whole arrays,
    heads included), the events, and whether every guard band is untouched."""
    from ofdm_sync_amd import _lib
    dev, g = bufs
    nb, t = x.shape[0], x.shape[2]
    out = {k: g[k].view(nb, t) for k in subset}
    n_ev = torch.zeros(nb, dtype=torch.int32, device=dev)
    ev_i = torch.zeros((nb, max_ev, 4), dtype=torch.int64, device=dev)
    ev_r = torch.zeros((nb, max_ev, 4), dtype=torch.float64, device=dev)
    ptr = lambda k: out[k].data_ptr() if k in out else None  # noqa: E731
    args = (_lib.C64, x.data_ptr(), nb, 1, t, L, _lib.FP32, ptr("P"), ptr("R"), ptr("M"), ptr("valid"), detect,
            float(thr), hyst, 15.36e6, max_ev, n_ev.data_ptr(), ev_i.data_ptr(), ev_r.data_ptr(),
            torch.cuda.current_stream().cuda_stream)
    with _lib.variants(**({} if full is None else {"FAST_FULL": full})):
        rc = _lib.lib().ofs_aa_detect(*args) if flags is None else _lib.lib().ofs_aa_detect_ex(*args, flags)
    assert rc == 0
    torch.cuda.synchronize()
    res = {k: v.clone() for k, v in out.items()}
    res.update(n_events=n_ev, ev_int=ev_i, ev_real=ev_r)
    return res, all(g[k].guards_intact() for k in subset)


def both_arms(bufs, x, L, what, keys=None, **kw):
    """Default dispatch against FAST_FULL = 0 on the same call: equal bits, guards intact; returns the
    default arm's result."""
    ref, intact = call(bufs, x, L, full=0, **kw)
    assert intact, (what, "FAST_FULL=0")
    got, intact = call(bufs, x, L, full=None, **kw)
    assert intact, (what, "default")
    for k in (keys or ref):
        assert torch.equal(bits(ref[k]), bits(got[k])), (what, k)
    return got


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("B", BS)
def test_full_stream_form_is_bit_identical(bufs, B, L):
    from ofdm_sync_amd import _lib
    assert _lib.lib().ofs_aa_plan(_lib.C64, _lib.FP32, 1, T, L) == 1020 + L // 128     # register-staged, E = 2
    x = device_batch(B, L)
    counts = {}
    for hyst in (128, 1, 16, 0):
        got = both_arms(bufs, x, L, ("head off", hyst), hyst=hyst)
        counts[hyst] = got["n_events"].cpu().numpy()
        assert counts[hyst][:B].sum() > 0                       # the streams do hold events
        # head flag on, heads left at the sentinel: the same bytes in both arms, P's head (and at the
        # headline's L = 512 also M's) not written at all
        got = both_arms(bufs, x, L, ("head on", hyst), hyst=hyst, flags=HEAD_FLAG)
        assert bool((bits(got["P"])[:, :L] == SENT32).all()), hyst
        if L == 512:
            assert bool((bits(got["M"])[:, :L] == SENT32).all()), hyst
        assert np.array_equal(got["n_events"].cpu().numpy(), counts[hyst])
        if hyst == 1 or (hyst, L) == (128, 512):                # gates open AND close inside the streams
            ends = got["ev_int"][3:B:4, 0, 2].cpu().numpy()
            assert (counts[hyst][3:B:4] >= 1).all(), hyst
            assert (ends < T - 1).all() if hyst == 1 else (ends < T - 1).any(), (hyst, ends)
    if L == 128:
        assert (counts[128][1:B:4] >= 2).all()                  # the two-burst streams: two gates each
    # one event slot on streams with two gates: the first event is stored, the count stays exact
    for hyst in (128, 1):
        got = both_arms(bufs, x, L, ("max_events 1", hyst), hyst=hyst, max_ev=1)
        assert np.array_equal(got["n_events"].cpu().numpy(), counts[hyst]), hyst


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("B", BS)
def test_threshold_edges(bufs, B, L):
    """thr exactly an M value, its float64 neighbours, and 0, 1.5, NaN: the fp32 compare of the
    full-stream form decides every sample as the generic form's fp64 compare does."""
    x = device_batch(B, L)
    first, _ = call(bufs, x, L, full=None)
    M = first["M"][:B, L:].cpu().numpy()
    inside = np.abs(np.where((M > 0.05) & (M < 0.95), M, 9.0) - 0.5)
    m = float(np.float64(M.flat[int(np.argmin(inside))]))      # an M[b][n] of a first run, mid-range
    assert 0.05 < m < 0.95
    for thr in (m, math.nextafter(m, math.inf), math.nextafter(m, -math.inf), 0.0, 1.5, math.nan):
        for hyst in (128, 1):
            got = both_arms(bufs, x, L, ("thr", thr, hyst), thr=thr, hyst=hyst)
            n = got["n_events"].cpu().numpy()
            if thr == 0.0:
                assert (n >= 1).all()                           # every sample is above
            if thr != thr or thr == 1.5:
                assert (n[:B] == 0).all()                       # none is (M <= 1)


@pytest.mark.parametrize("L", LS)
def test_other_calls_are_unaffected(bufs, L):
    """Calls the full-stream form does not cover: the variant must change nothing."""
    B = BS[0]
    x = device_batch(B, L)
    for subset in (("R",), ("P", "M"), ("P", "R", "M", "valid")):
        both_arms(bufs, x, L, subset, subset=subset)
        both_arms(bufs, x, L, (subset, "head"), subset=subset, flags=HEAD_FLAG)
    both_arms(bufs, x, L, "detect off", detect=0)
    for t in (1022, 640):
        both_arms(bufs, device_batch(B, L, t), L, ("T", t))
        both_arms(bufs, device_batch(B, L, t), L, ("T", t, "head"), flags=HEAD_FLAG)


@pytest.mark.parametrize("L", LS)
def test_default_arm_matches_oracle(bufs, L):
    import oracle_c
    import parity
    B = BS[0]
    xh = np.ascontiguousarray(batch(B, L)[:B])                   # without the NaN / Inf stream
    o = oracle_c.aa_detect(xh, L, max_events=E, nthreads=4)
    got, intact = call(bufs, device_batch(B, L)[:B].contiguous(), L, full=None)
    assert intact
    r = parity.classify_aa(got["M"].cpu().numpy().astype(np.float64), got["n_events"].cpu().numpy(),
                           got["ev_int"].cpu().numpy(), got["ev_real"].cpu().numpy(), o["P"], o["M"],
                           o["n_events"], o["ev_int"], o["ev_real"], L)
    print("full-stream parity", L, r)
    assert r["mismatch"] == 0, r
    assert r["cfo_over_tol"] == 0, r
    assert r["max_abs_err_M"] <= 1e-6, r
    assert int(o["n_events"].sum()) > 0
