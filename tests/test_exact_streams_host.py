"""CPU: the exact-arithmetic stream sets of tests/exact_streams.py are what they claim to be.

For every (L, T, n_ant) that tests/test_gpu_aa_exact_events.py uses and every hysteresis of its list:
check() passes (integer P and R on an axis, every |M - thr| >= 1e-4, and the coverage of the gate
machine's edges that the shape can hold), the prefix-sum oracle, the literal-loop oracle and the C
oracle agree exactly on P, R and the event integers (P lies on an axis, so the C oracle's hypot is
exact), and the integer values survive complex64, int16 and the packed 12-bit words.
"""
import numpy as np
import pytest

import exact_streams as X
import ofdm_oracle as O
import oracle_c
from ofdm_sync_amd import wire


@pytest.mark.parametrize("L,T,n_ant", X.all_shapes(), ids=lambda v: str(v))
def test_preconditions_and_coverage(L, T, n_ant):
    worst = 1.0
    for hyst in X.hysts(T):
        r = X.check(L, T, hyst, n_ant)
        worst = min(worst, r["margin"])
    print(f"L={L} T={T} n_ant={n_ant}: min |M - thr| = {worst:.3e}")
    assert worst >= X.MARGIN


@pytest.mark.parametrize("L,T,n_ant", X.all_shapes(), ids=lambda v: str(v))
def test_oracles_agree(L, T, n_ant):
    """The three oracles on the stream sets of three hysteresis values (the sets differ with it; the
    metric does not depend on it, and aa_events is one function for both Python oracles)."""
    for hyst in (X.hysts(T)[1], 128, X.hysts(T)[-1]):
        names, iq = X.streams(L, T, hyst, n_ant)
        orc = X.oracle(L, T, hyst, n_ant)
        x = X.cplx(iq)
        c = oracle_c.aa_detect(x, L, X.THR, hyst, X.FS, max_events=64, nthreads=2)
        for b in range(len(names)):
            P, R, M, valid, ei, er = orc[b]
            Pl, Rl, Ml, vl = O.aa_metric_loop(x[b], L)
            assert np.array_equal(P, Pl) and np.array_equal(R, Rl) and np.array_equal(M, Ml), names[b]
            assert np.array_equal(valid, vl), names[b]
            assert np.array_equal(c["P"][b], P) and np.array_equal(c["R"][b], R), names[b]
            assert c["n_events"][b] == len(ei), names[b]
            assert np.array_equal(c["ev_int"][b, :len(ei)], ei), names[b]
            assert np.array_equal(c["ev_real"][b, :len(ei), :2], er[:, :2]), names[b]
        # one literal-loop detection end to end
        b = len(names) // 2
        got = O.aa_detect_loop(x[b], L, X.THR, hyst, X.FS)
        assert np.array_equal(got[4], orc[b][4]) and np.array_equal(got[5], orc[b][5])


def test_values_survive_every_input_format():
    names, iq = X.streams(128, 1024, 16, 2)
    x = X.cplx(iq)
    assert np.array_equal(x.astype(np.complex64).astype(np.complex128), x)
    assert np.array_equal(wire.unpack_axis(wire.pack_axis(iq)), iq)
    assert set(np.unique(iq).tolist()) <= {-1, 0, 1}


def test_rotation_streams_give_the_stated_events():
    """The block-rotation and zero-head streams at L = 128, T = 1024: P on the imaginary / negative
    real axis with Im P = +0.0, the CFO exactly fs / (4L) and fs / (2L) (angle +pi), every sample
    from 2L - 1 on a tie with the peak; the zero head opens at n = L and R falls to exactly 0."""
    L, T, hyst = 128, 1024, 16
    names, iq = X.streams(L, T, hyst)
    orc = X.oracle(L, T, hyst)
    P, R, M, valid, ei, er = orc[names.index("rot_j")]
    assert ei.tolist() == [[255, 177, 1024, 255 - 2 * L + 1]]
    assert er[0, 0] == 0.0 and er[0, 1] == 128.0 and er[0, 3] == X.FS / (4 * L) == 30000.0
    assert np.all(np.abs(P[255:]) ** 2 == 128.0 ** 2)
    P, R, M, valid, ei, er = orc[names.index("rot_neg")]
    assert er[0, 0] == -128.0 and er[0, 1] == 0.0 and not np.signbit(er[0, 1])
    assert er[0, 3] == np.pi * X.FS / (2 * np.pi * L) and er[0, 3] > 0
    P, R, M, valid, ei, er = orc[names.index("zero_head")]
    assert ei.tolist() == [[128, 128, 271, 128 - 2 * L + 1]]
    assert R[2 * L] == 0.0 and M[2 * L] == 0.0 and M[L] == 1.0 and not np.any(np.isnan(M))
