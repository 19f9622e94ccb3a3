"""The resident P/M head of the fp32 [A][A] fast paths (ofs_aa_detect_ex, OFS_AA_HEAD_RESIDENT).

P[n] and M[n] of n < L are +0.0 for any input, so a caller whose buffers already hold those zeros
may let the library leave them unwritten.  The kernels are called through the C ABI so that the
test owns the buffers: every output is a view into a larger allocation with 2 KiB of sentinel bytes
on both sides, and a view is filled with the sentinel before each call, so a byte the kernel did not
write is still the sentinel afterwards.

B = 5 (odd streams make b*T only 8-byte aligned), inputs from test_gpu_store_path.stream_batch
(gates and events in the longer streams).  Register-staged kernel: L = 128, 256, 384 (three rows: a
row pair straddles the head boundary), 512 with the stream lengths of test_gpu_store_path; streaming
kernel: T = 1030, 2049 with L = 128, 512 and one or two antennas.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_gpu_store_path import stream_batch

gpu = pytest.mark.gpu

B = 5
E = 4                                   # max_events
GUARD = 2048
SENTINEL = 0xA5
SENT32 = int(np.frombuffer(bytes([SENTINEL] * 4), dtype=np.int32)[0])
DTYPES = {"P": torch.complex64, "R": torch.float32, "M": torch.float32, "valid": torch.uint8}
SUBSETS = (("P", "R", "M"), ("P",), ("M",), ("R",), ("P", "M", "valid"))
TMAX = 2049
HEAD_FLAG = 1                           # OFS_AA_HEAD_RESIDENT

REG_SHAPES = [(T, L, 1) for L in (128, 256, 384, 512) for T in (1024, 1022, 640, 516, 256, 128, 4, 2)]
STREAM_SHAPES = [(T, L, na) for T in (1030, 2049) for L in (128, 512) for na in (1, 2)]
SHAPES = REG_SHAPES + STREAM_SHAPES


@functools.lru_cache(maxsize=None)
def batch(T, L, na):
    """[B, na, T] complex64 (host); the second antenna is the first one's batch in reverse stream order."""
    x = stream_batch(T, L)
    if na == 2:
        x = np.concatenate([x, 0.5 * x[::-1]], axis=1)
    return np.ascontiguousarray(x)


class Guarded:
    """An output array as a view into a larger allocation, sentinel bytes everywhere around it."""

    def __init__(self, dtype, dev):
        self.raw = torch.empty(B * TMAX * 8 + 2 * GUARD, dtype=torch.uint8, device=dev)
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


def bits(t):
    """Integer view of a tensor (bit comparison: NaN-safe, signed zeros told apart)."""
    if t.is_complex():
        t = torch.view_as_real(t)
    if t.is_floating_point():
        t = t.view(torch.int32 if t.element_size() == 4 else torch.int64)
    return t


def plan_of(T, L, na):
    from ofdm_sync_amd import _lib
    return int(_lib.lib().ofs_aa_plan(_lib.C64, _lib.FP32, na, T, L))


def call(bufs, x, T, L, na, subset, flags, zero_head=False, **variants):
    """One call into guarded, sentinel-filled buffers (flags None: plain ofs_aa_detect).  zero_head:
    the P and M heads are zeroed first (the state the flag promises).  Returns outputs + events and
    whether every guard band is untouched."""
    from ofdm_sync_amd import _lib
    dev, g = bufs
    xd = torch.from_numpy(x).to(dev)
    out = {k: g[k].view(T) for k in subset}
    if zero_head:
        for k in ("P", "M"):
            if k in out:
                out[k][:, :min(L, T)] = 0
    n_ev = torch.zeros(B, dtype=torch.int32, device=dev)
    ev_i = torch.zeros((B, E, 4), dtype=torch.int64, device=dev)
    ev_r = torch.zeros((B, E, 4), dtype=torch.float64, device=dev)
    ptr = lambda k: out[k].data_ptr() if k in out else None  # noqa: E731
    args = (_lib.C64, xd.data_ptr(), B, na, T, L, _lib.FP32, ptr("P"), ptr("R"), ptr("M"), ptr("valid"), 1, 0.15,
            128, 15.36e6, E, n_ev.data_ptr(), ev_i.data_ptr(), ev_r.data_ptr(), torch.cuda.current_stream().cuda_stream)
    with _lib.variants(**variants):
        rc = _lib.lib().ofs_aa_detect(*args) if flags is None else _lib.lib().ofs_aa_detect_ex(*args, flags)
    assert rc == 0
    torch.cuda.synchronize()
    res = {k: v.clone() for k, v in out.items()}
    res.update(n_events=n_ev, ev_int=ev_i, ev_real=ev_r)
    return res, all(g[k].guards_intact() for k in subset)


def check_shape(T, L, na):
    plan = plan_of(T, L, na)
    if L == 384 and not 1000 <= plan < 1200:
        pytest.skip(f"L = 384 not on the fast path (plan {plan})")
    assert 1000 <= plan < 1200, plan
    assert (plan < 1100) == (T <= 1024), plan           # register-staged / streaming as intended


@gpu
@pytest.mark.parametrize("T,L,na", SHAPES)
def test_zeroed_head_with_flag_is_bit_identical_to_plain(bufs, T, L, na):
    check_shape(T, L, na)
    x = batch(T, L, na)
    for subset in SUBSETS:
        ref, intact = call(bufs, x, T, L, na, subset, None)
        assert intact, subset
        got, intact = call(bufs, x, T, L, na, subset, HEAD_FLAG, zero_head=True)
        assert intact, subset
        for k in ref:
            assert torch.equal(bits(ref[k]), bits(got[k])), (subset, k)


@gpu
@pytest.mark.parametrize("T,L,na", SHAPES)
def test_sentinel_head_with_flag(bufs, T, L, na):
    """Head left at the sentinel: n >= L as the plain call, every head element the sentinel or +0.0;
    on the headline's kernel shape the head is not written at all; variant FAST_HEAD = 0 writes it."""
    check_shape(T, L, na)
    x = batch(T, L, na)
    h = min(L, T)
    for subset in SUBSETS:
        ref, intact = call(bufs, x, T, L, na, subset, None)
        assert intact, subset
        got, intact = call(bufs, x, T, L, na, subset, HEAD_FLAG)
        assert intact, subset
        for k in ref:
            a, b = bits(ref[k]), bits(got[k])
            if k in ("P", "M"):
                assert torch.equal(a[:, h:], b[:, h:]), (subset, k)
                head = b[:, :h]
                assert bool(((head == SENT32) | (head == 0)).all()), (subset, k)
                if (T, L, na) == (1024, 512, 1):
                    assert bool((head == SENT32).all()), (subset, k)     # the bytes are no longer written
            else:
                assert torch.equal(a, b), (subset, k)
        off, intact = call(bufs, x, T, L, na, subset, HEAD_FLAG, FAST_HEAD=0)
        assert intact, subset
        for k in ref:
            assert torch.equal(bits(ref[k]), bits(off[k])), (subset, k)
            if k in ("P", "M"):
                assert bool((bits(off[k])[:, :h] == 0).all()), (subset, k)


@gpu
@pytest.mark.parametrize("T,L,na", [(1024, 512, 1), (1024, 384, 1), (1022, 128, 1), (640, 256, 1), (1030, 128, 2),
                                    (2049, 512, 1), (2049, 512, 2)])
def test_plain_call_writes_a_zero_head_for_any_input(bufs, T, L, na):
    """The invariant the flag rests on: NaN, Inf and 1e30 among the first L samples leave all-zero
    bits in P[:, :L] and M[:, :L] of a plain call."""
    check_shape(T, L, na)
    x = batch(T, L, na).copy()
    for b_ in range(B):
        for t in range(na):
            x[b_, t, (3 + 5 * b_ + t) % L] = np.nan
            x[b_, t, (17 + b_ + 2 * t) % L] = complex(np.inf, -1.0)
            x[b_, t, (40 + 7 * b_) % L] = complex(1e30, -1e30)
            x[b_, t, L - 1] = complex(-np.inf, np.nan)
    got, intact = call(bufs, x, T, L, na, ("P", "R", "M"), None)
    assert intact
    for k in ("P", "M"):
        assert bool((bits(got[k])[:, :L] == 0).all()), k


DET_SHAPES = [(1024, 512, 1), (2049, 512, 2)]


@gpu
@pytest.mark.parametrize("T,L,na", DET_SHAPES)
@pytest.mark.parametrize("rewrite_head", (False, True))
def test_batch_detector_matches_the_one_shot_call(T, L, na, rewrite_head):
    """AABatchDetector on batch A, then on another batch B: B's result is the one-shot function's,
    bit for bit, heads included (events: the live slots)."""
    from ofdm_sync_amd import sync_aa
    dev = torch.device("cuda", 0)
    xa = torch.from_numpy(batch(T, L, na)).to(dev)
    xb = torch.from_numpy(np.ascontiguousarray(1.5 * np.roll(batch(T, L, na)[::-1], 7, axis=2))).to(dev)
    det = sync_aa.AABatchDetector(B, T, na, L, outputs=("P", "R", "M"), max_events=E, rewrite_head=rewrite_head,
                                  device=dev)
    assert 1000 <= det.plan() < 1200
    assert det.head_resident == (not rewrite_head)
    det.x.copy_(xa)
    det.run()
    res = det.run(xb)
    ref = sync_aa.aa_detect_streaming_batched(xb, L, outputs=("P", "R", "M"), max_events=E)
    torch.cuda.synchronize()
    for k in ("P", "R", "M", "n_events"):
        assert torch.equal(bits(getattr(res, k)), bits(getattr(ref, k))), k
    n = np.minimum(ref.n_events.cpu().numpy(), E)            # live slots (the rest is never written)
    assert n.sum() > 0                                       # batch B does hold events
    for b_ in range(B):
        for k in ("ev_int", "ev_real"):
            assert torch.equal(bits(getattr(res, k)[b_, :n[b_]]), bits(getattr(ref, k)[b_, :n[b_]])), (k, b_)


# ---- host (no GPU): the flags entry point ----
def test_flags_entry_is_declared_and_refuses_unknown_bits():
    hdr = open(os.path.join(ROOT, "include", "ofdmsync.h")).read()
    assert re.search(r"^int32_t\s+ofs_aa_detect_ex\s*\(", hdr, re.M)
    assert re.search(r"^#define\s+OFS_AA_HEAD_RESIDENT\s+1u?\s*$", hdr, re.M)
    path = os.path.join(ROOT, "ofdm-sync-math_amd", "ofdm_sync_amd", "libofdmsync.so")
    if not os.path.exists(path):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(path)
    from ofdm_sync_amd import _lib as L_
    L_._declare(lib)
    a = (0, 1, 1, 1, 1024, 512, 0, None, None, None, None, 0, 0.15, 128, 15.36e6, 0, None, None, None, None)
    for bad in (2, 3, 0x80000000, 0xFFFFFFFE):
        assert lib.ofs_aa_detect_ex(*a, bad) == -1, bad          # refused before anything is launched
    # known flags pass validation: an empty batch is a valid no-op with or without the flag
    e = (0, None, 0, 1, 1024, 512, 0, None, None, None, None, 1, 0.15, 128, 15.36e6, 4, None, None, None, None)
    assert lib.ofs_aa_detect_ex(*e, 0) == 0
    assert lib.ofs_aa_detect_ex(*e, HEAD_FLAG) == 0
    assert lib.ofs_aa_detect_ex(0, None, 1, 1, 1024, 512, 0, None, None, None, None, 0, 0.15, 128, 15.36e6, 0,
                                None, None, None, None, HEAD_FLAG) == -1    # other checks still apply
