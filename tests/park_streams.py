"""Small exact streams for the running peak of the chunked Park metric (park.ParkChunkedMetric).

``tie_stream`` is int16 I/Q, so P, E and M of oracle/ofdm_oracle.py:park_metric and of the fp64 kernels
are exact and a tie is a tie in every bit; ``nan_stream`` is complex64 with one NaN sample.
tests/test_park_streams_host.py proves on the CPU that the streams hold what is claimed here;
tests/test_gpu_park_chunked.py feeds them to the GPU in the chunkings given below.
"""
from __future__ import annotations

import numpy as np

# ---- tie stream ---------------------------------------------------------------------------------
TIE_N = 64                                   # half = 32
TIE_T = 600
TIE_STARTS = ((100, 300, 480), (93, 305, 471))     # first sample of each block, per stream
TIE_CHUNKS = (150, 97, 113, 77, 163)               # the pushes of the GPU test (sum = TIE_T)


def tie_centres(row: int) -> list[int]:
    """The reference's centre index d of each block of stream ``row``."""
    return [s + TIE_N // 2 - 1 for s in TIE_STARTS[row]]


def tie_stream() -> np.ndarray:
    """int16 [2, 1, TIE_T, 2].  Complex noise, I and Q uniform in [-100, 100], with three copies of ONE
    real-valued block of 2 * half - 1 samples, mirror-symmetric about its middle (values uniform in
    [-200, 200], never 0).  At a block's centre d every product x[d-k] * x[d+k] is the square
    x[d+k]^2, so P = E exactly and M = 1.0; everywhere else M < 1 (checked on the host)."""
    rng = np.random.default_rng(20240611)
    half = TIE_N // 2
    side = rng.integers(20, 201, half) * rng.choice([-1, 1], half)       # the centre and the right half
    block = np.concatenate([side[:0:-1], side])                          # 2 * half - 1, symmetric
    assert block.size == 2 * half - 1 and np.array_equal(block, block[::-1])
    x = rng.integers(-100, 101, (2, 1, TIE_T, 2))
    for row, starts in enumerate(TIE_STARTS):
        for s in starts:
            x[row, 0, s:s + block.size, 0] = block
            x[row, 0, s:s + block.size, 1] = 0
    return x.astype(np.int16)


# ---- NaN stream ---------------------------------------------------------------------------------
NAN_N = 64
NAN_T = 700
NAN_AT = 250                                 # the NaN sample
NAN_BLOCK = 450                              # first sample of a symmetric block behind it
NAN_CHUNKS = (120, 95, 101, 184, 200)              # the pushes of the GPU test (sum = NAN_T)


def nan_first_d() -> int:
    """d of the first output whose window x[d-half+1 .. d+half-1] holds the NaN sample."""
    return NAN_AT - (NAN_N // 2 - 1)


def nan_stream() -> np.ndarray:
    """complex64 [2, 1, NAN_T].  Stream 0: unit-variance noise, one NaN sample at NAN_AT and, well behind
    it, a real symmetric block of amplitude 1.5 whose centre has M close to 1: a larger number than any
    M before the NaN, which must not replace it.  Stream 1: the same without the NaN."""
    rng = np.random.default_rng(7)
    half = NAN_N // 2
    x = (rng.standard_normal((2, 1, NAN_T)) + 1j * rng.standard_normal((2, 1, NAN_T))) / np.sqrt(2.0)
    side = 1.5 * rng.choice([-1.0, 1.0], half)
    block = np.concatenate([side[:0:-1], side])
    x[:, 0, NAN_BLOCK:NAN_BLOCK + block.size] = block
    x[1] = x[0]
    x = x.astype(np.complex64)
    x[0, 0, NAN_AT] = np.float32("nan")
    return x


def call_of_sample(chunks, n: int) -> int:
    """Index of the push that holds sample n."""
    edge = np.cumsum(chunks)
    assert 0 <= n < edge[-1]
    return int(np.searchsorted(edge, n, side="right"))


def call_of_d(chunks, d: int, N: int) -> int:
    """Index of the push after which the running peak covers centre index d: the one that brings sample
    d + half, with which the reference has output d.  (Its window ends one sample earlier; d + half - 1
    and d + half lie in the same push for every index the tests ask about, which the host test checks.)"""
    assert call_of_sample(chunks, d + N // 2 - 1) == call_of_sample(chunks, d + N // 2)
    return call_of_sample(chunks, d + N // 2)
