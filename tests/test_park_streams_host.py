"""CPU: the streams of tests/park_streams.py hold what they claim, by oracle/ofdm_oracle.py:park_metric
(float64 on integer samples: P, E and the ties are exact)."""
import numpy as np

import ofdm_oracle as O
import park_streams as PS


def _iq(x):
    return x[..., 0].astype(np.float64) + 1j * x[..., 1].astype(np.float64)


def test_tie_stream_has_three_exact_ties_in_different_calls():
    x = PS.tie_stream()
    assert x.shape == (2, 1, PS.TIE_T, 2) and x.dtype == np.int16 and sum(PS.TIE_CHUNKS) == PS.TIE_T
    N, half = PS.TIE_N, PS.TIE_N // 2
    for row in range(2):
        ds, M, P, E = O.park_metric(_iq(x[row]), N)
        assert ds[0] == half and ds.size == PS.TIE_T - 2 * half
        centres = PS.tie_centres(row)
        # the global maximum sits at exactly the three designed centres, with equal bits (1.0)
        top = np.flatnonzero(M == M.max())
        assert (ds[top]).tolist() == centres, (row, ds[top], centres)
        bits = M[top].view(np.int64)
        assert M.max() == 1.0 and np.all(bits == bits[0])
        assert np.all(P[top].imag == 0.0) and np.array_equal(P[top].real, E[top])
        # the tied maxima fall in different pushes of the GPU test's chunking
        calls = [PS.call_of_d(PS.TIE_CHUNKS, d, N) for d in centres]
        assert len(set(calls)) == 3 and calls == sorted(calls), calls
        # an earlier, smaller local maximum exists: the running peak of the pushes before the first
        # centre's is a number below 1 at another index, which the first centre must replace
        assert calls[0] >= 1
        seen = sum(PS.TIE_CHUNKS[:calls[0]]) - 2 * half                  # the reference's outputs before that push
        assert seen > 2
        j = int(np.argmax(M[:seen]))
        assert 0 < j < seen - 1 and 0.0 < M[j] < 1.0 and M[j - 1] < M[j] > M[j + 1], (row, j, M[j])
        # everything is an exact integer in float64
        assert np.all(E == np.round(E)) and np.all(P.real == np.round(P.real)) and E.max() < 2.0 ** 40


def test_nan_stream_first_nan_and_a_larger_number_behind_it():
    x = PS.nan_stream()
    assert x.shape == (2, 1, PS.NAN_T) and x.dtype == np.complex64 and sum(PS.NAN_CHUNKS) == PS.NAN_T
    N, half = PS.NAN_N, PS.NAN_N // 2
    assert np.flatnonzero(np.isnan(x[0, 0].real)).tolist() == [PS.NAN_AT] and not np.isnan(x[1]).any()
    ds, M, P, E = O.park_metric(x[0].astype(np.complex128), N)
    nan = np.flatnonzero(np.isnan(M))
    # the first NaN of M is the first output whose window x[d-half+1 .. d+half-1] holds the sample
    # (the oracle's E is a difference of prefix sums, so its M stays NaN from there on: the outputs
    # behind the sample are taken from the oracle on the rest of the stream, which has the same windows)
    assert ds[nan[0]] == PS.nan_first_d() == PS.NAN_AT - half + 1 and np.argmax(M) == nan[0]   # numpy: the first NaN wins
    before = M[:nan[0]].max()
    rest = PS.NAN_AT + 1
    ds2, after, _, _ = O.park_metric(x[0, :, rest:].astype(np.complex128), N)
    ds2 = ds2 + rest
    jmax = int(np.argmax(after))
    assert np.isfinite(after).all() and after.max() > before > 0.0
    assert ds2[jmax] == PS.NAN_BLOCK + half - 1 and abs(after.max() - 1.0) < 1e-5
    # the NaN and the larger number behind it arrive in different pushes, the NaN not in the first
    c_nan = PS.call_of_d(PS.NAN_CHUNKS, int(ds[nan[0]]), N)
    c_max = PS.call_of_d(PS.NAN_CHUNKS, int(ds2[jmax]), N)
    assert 1 <= c_nan < c_max, (c_nan, c_max)
    # the stream without the NaN peaks at the block
    ds1, M1, _, _ = O.park_metric(x[1].astype(np.complex128), N)
    assert ds1[int(np.argmax(M1))] == PS.NAN_BLOCK + half - 1
