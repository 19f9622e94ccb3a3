"""CPU: the exact matched-filter streams of tests/zc_mf_streams.py hold what they claim, and the checker
the GPU tests use (zc_mf_streams.check) rejects every mutant of a numpy model on every stream family.

(a) Every partial sum of corr and of the window energy is an integer below 2^53, so fp64 FMA chains are
    exact in any order; the straddle energies 0, 1, 4, 5, 8 (x 2^-42) exist on both sides of 1e-12; the
    zero span gives windows of energy exactly 0; for each length the block seams fall where stated.
(b) numpy's fp64 FFT overlap-save with the reference's float64 normaliser passes the per-block checker at
    4e-6 to 2.5e-5 of the bound of error model 4 (0.011 to 0.066 of u·log2(M)·||u_q||·||ref||; printed).  Each
    mutant of it - outputs shifted by one sample, a block's outputs taken from its neighbour, one RAW word
    off by 1, the window energy over N - 1 or N + 1 samples, the conjugate dropped, the taps not reversed,
    branch 1 ignored, V2's per-branch normalisation exchanged with COMBINED's summed one, 1e-9 of the row
    maximum added inside a quiet block - is rejected in at least one mode on every family.
    The present criterion of tests/test_gpu_corr.py ("1e-11 of the row maximum", |corr| rtol 1e-9) also
    rejects an error of 1e-9 of the row maximum - it is a hundred times its own tolerance - so the gap is
    shown with half that tolerance: 5e-12 of the row maximum inside a quiet block of the loud stream passes
    the present criterion and is 139 times outside the per-block bound.
"""
import numpy as np
import pytest

import error_models as EM
import zc_mf_streams as Z

MODES = (Z.RAW, Z.SUM, Z.V2, Z.COMBINED)


def test_streams_hold_what_they_claim():
    for fam, N, T in Z.cases() + [("straddle", 2048, 10243)]:
        st = Z.stream(fam, N, T)
        f = Z.facts(st)
        print(f"{st.name}: largest partial sum 2^{np.log2(max(f['partial'], 1)):.1f}, zero-energy windows {f['zero_windows']}")
        assert f["partial"] < 2 ** 53
        assert np.abs(st.xr).max() <= 32767 and np.abs(st.xi).max() <= 32767
        if fam == "zero":
            a, b = Z.zero_span(N, T)
            assert b - a > N and f["zero_windows"] == b - a - N + 1
            seam = Z.pick_m(N, T, 1) - N + 1                  # the zero-energy outputs lie on both sides of a seam
            assert a + N - 1 < seam < b - 1
        if fam == "straddle":
            assert {0, 1, 4, 5, 8} <= f["energies"]
            assert 4 * 2.0 ** -42 < 1e-12 < 5 * 2.0 ** -42
            cr, ci, e = st.exact()
            for k in (4, 5):                                  # a non-zero corr on either side of the clamp
                assert ((e[0] == k) & ((cr[0] != 0) | (ci[0] != 0))).any()
        if fam == "loud" and N == Z.N_BIG:
            assert {tuple(Z.blocks_holding(s, N, Z.M_BIG, st.nout)) for s in (Z.LOUD_AT, Z.LOUD_AT + Z.LOUD_LEN - 1)} == {(1,)}
    # the inexact stream: corr's partial sums stay below 2^53, the energy's do not
    st = Z.stream("inexact", 2048, 16384)
    rr, ri = Z.taps(2048)
    h = (np.abs(rr) + np.abs(ri))[::-1].astype(np.int64)
    assert max(int(np.convolve(np.abs(a) + np.abs(b), h).max()) for a, b in zip(st.xr, st.xi)) < 2 ** 53
    assert int(st.exact()[2].max()) > 2 ** 53
    assert np.abs(Z.ref_c(2048)).max() > 0 and Z.taps(300)[0].size == 300


def test_seams_fall_where_stated():
    S = Z.S_BIG
    assert S == 6145
    want = {10243: (2, S), 10244: (3, 1), 16384: (3, 16384 + 2047 - 2 * S), 1000: (1, 3047), 1: (1, 2048)}
    for T, (nblk, last) in want.items():
        nout = T + Z.N_BIG - 1
        assert -(-nout // S) == nblk and nout - (nblk - 1) * S == last, T
    for N in (256, 300):
        assert Z.pick_m(N, 3000, 1) == Z.pick_m(N, 3000, 3) == 2048        # the rocFFT pipeline, 2 blocks


def test_numpy_models_pass_the_checker():
    """numpy's overlap-save against the per-block bound and numpy's exact integer convolution with the
    reference's float64 normaliser against the direct kernel's criterion, every case, 2 branches."""
    worst, worst_d = 0.0, 0.0
    for fam, N, T in Z.cases() + [("straddle", 2048, 10243)]:
        st = Z.stream(fam, N, T)
        M = Z.pick_m(N, T, 2)
        for mode in MODES:
            corr, mag = Z.os_model(st, 2, mode, M)
            v = Z.check(st, 2, mode, corr, mag, "numpy", M)
            assert v, (st.name, mode, v.why)
            worst = max(worst, v.ratio if mode == Z.RAW else 0.0)
            ex = Z.expected(st, 2, mode)
            if mode in (Z.RAW, Z.SUM):
                d = (ex.re + 1j * ex.im).astype(np.complex128)
            else:
                cr, ci, e = (np.ldexp(a[:2].astype(np.float64), s) for a, s in zip(st.exact(), (st.shift, st.shift, 2 * st.shift)))
                rn = np.sqrt(Z.ref_energy(N))
                d = ((cr + 1j * ci).sum(0) / (rn * np.sqrt(np.maximum(e.sum(0), 0.0) + 1e-12)) if mode == Z.COMBINED
                     else ((cr + 1j * ci) / (rn * np.sqrt(np.maximum(e, 1e-12)))).sum(0))[None]
            vd = Z.check(st, 2, mode, d, np.hypot(d.real, d.imag), "direct", exp=ex)
            assert vd, (st.name, mode, vd.why)
            worst_d = max(worst_d, vd.ratio)
    K = EM.zc_os_K(Z.ref_c(2048), 8192, "numpy")
    print(f"numpy overlap-save: worst |error| / bound {worst:.3g} (K = {K:.0f}: {worst * K:.3g} of u·L·|u_q|·|ref|); "
          f"float64 normaliser on exact integers: {worst_d:.3g} of the direct criterion")
    assert worst < 1e-4


FAMILY_STREAMS = [("noise", 2048, 16384), ("zero", 2048, 16384), ("loud", 2048, 16384), ("straddle", 2048, 10243),
                  ("noise", 300, 3000), ("loud", 256, 3000), ("zero", 300, 3000)]


@pytest.mark.parametrize("fam,N,T", FAMILY_STREAMS)
def test_every_mutant_is_rejected(fam, N, T):
    st = Z.stream(fam, N, T)
    M = Z.pick_m(N, T, 2)
    for mut in Z.MUTANTS:
        hit = []
        for mode in MODES:
            corr, mag = Z.os_model(st, 2, mode, M, mut)
            v = Z.check(st, 2, mode, corr, mag, "numpy", M)
            if not v:
                hit.append((Z.MODE_NAME[mode], f"{v.ratio:.3g}"))
        print(f"{st.name} {mut}: rejected in {hit}")
        assert hit, (st.name, mut)


def test_quiet_block_error_passes_the_present_criterion_only():
    st = Z.stream("loud", 2048, 16384)
    q = Z.quiet_block(st, Z.M_BIG)
    assert q != 1                                             # the burst's block is not the quiet one
    for mut, old_accepts in ((None, True), (Z.GAP_MUTANT, True), ("quiet_block_1e-9", False)):
        corr, mag = Z.os_model(st, 1, Z.RAW, Z.M_BIG, mut)
        ex = Z.expected(st, 1, Z.RAW)
        v = Z.check(st, 1, Z.RAW, corr, mag, "numpy", Z.M_BIG)
        print(f"{mut}: present criterion accepts {Z.old_criterion(corr, mag, ex)}, per-block ratio {v.ratio:.3g}")
        assert Z.old_criterion(corr, mag, ex) == old_accepts
        assert bool(v) == (mut is None)
    assert v.ratio > 10


def test_rsqrt_newton_within_its_constant():
    w = EM.rsqrt_newton_worst()
    print(f"two Newton steps from a 2^-23 seed: {w:.3f} u")
    assert w <= EM.ZC_RSQRT_U


def test_batch_moves_content_across_every_seam_and_shifts_exactly():
    plan = Z.batch_plan()
    assert len(plan) == Z.BATCH_B and {k for k, _, _ in plan} == {0, 1, 2} and {r for _, _, r in plan} == {0, 1, 2, 3}
    for k in range(3):
        ds = {d for kk, d, _ in plan if kk == k}
        assert ds == set(Z.BATCH_DELAYS), k
    S = Z.S_BIG
    burst = {Z.BATCH_BURST_AT + d for d in Z.BATCH_DELAYS}
    L = Z.LOUD_LEN
    for seam in (S, 2 * S - (Z.N_BIG - 1)):                   # the outputs' seam, the third span's start
        assert any(b + L <= seam for b in burst) and any(b < seam < b + L for b in burst), seam
    assert any(b >= S for b in burst)
    for b in (7, 100):                                         # shifting the expectation = recomputing it
        ex, st = Z.batch_expected(b, Z.V2), Z.batch_stream(b)
        ex2 = Z.expected(st, 1, Z.V2)
        assert np.array_equal(ex.re, ex2.re) and np.array_equal(ex.im, ex2.im) and np.array_equal(ex.e, ex2.e)
    assert Z.batch_x().shape == (Z.BATCH_B, 1, Z.BATCH_T)
