"""GPU: the ZC matched filter and its normaliser on the exact streams of tests/zc_mf_streams.py.

Direct kernel (corr.hip zc_mf_kernel, method="direct").  Samples and taps are integers and every partial
sum is below 2^53 (tests/test_zc_mf_streams_host.py), so its FMA chains are exact in any order:
  RAW / SUM   corr bit for bit the integers of four int64 convolutions, head (n < N - 1) and tail (n >= T)
              included, every format, branch count, length and N; |corr| within 1 ulp of the correctly
              rounded root (the device hypot is not proven correctly rounded);
  V2 / COMBINED / NORMALIZE   every component within k·u (u = 2^-53, so at most k ulp) of the exact value
              evaluated in longdouble from those integers, k = 5 for one branch: the kernel's sequence
              (corr.hip:129-148) is the host's sqrt(ref_energy) 1, the device sqrt 2 (taken within 1 ulp),
              the product 1, the division 1; each further branch adds 1 (its add), COMBINED adds 1 for
              e + 1e-12 (error_models.zc_norm_k).  Measured: see DESIGN.md §4.5b;
  the zero span gives exactly +0.0 in every normalised mode; the straddle stream takes the reference's
  side of max(e, 1e-12) at 4·2^-42 and at 5·2^-42 (the two sides differ by 5 % there, k·u apart they are not).

Overlap-save kernels (method="fft": the persistent kernel, variant MC_PERS=0 the one-block kernel, variant
MC_FUSED=0 the rocFFT pipeline).  For block q with input span u_q every output meets error model 4:
  |d corr| <= K·u·log2(M)·||u_q||_2·||ref||_2, K from error_models.zc_os_K (about 2900 for these taps),
asserted per block as max |error| / bound <= 1 and printed, no output skipped.  On the loud stream the energy
prefix is still exact (integers below 2^53), so the same bound, propagated through the exact window energy,
plus the counted roundings of each kernel's normaliser holds in the normalised modes.  The inexact stream
(2^27 next to 1 in one block) is checked against |d e| <= ZC_OS_KE·u·E_block, the model in the header of
zc_fftcorr.hip; the direct kernel is still exact there in RAW and SUM.

Non-finite samples spoil what their window (direct) or their block (overlap-save) holds and nothing else;
|corr| up to 1e200 stays finite; a window whose energy overflows gives 0 (zc_v2.py:269-271).
"""
import numpy as np
import pytest

import error_models as EM
import zc_mf_streams as Z

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from ofdm_sync_amd import _lib, zc_v2  # noqa: E402

MODES = (Z.RAW, Z.SUM, Z.V2, Z.COMBINED)
KERNELS = {"pers": {}, "fused": {"MC_PERS": 0}, "rocfft": {"MC_FUSED": 0}}
_plans: dict = {}


def to_dev(x):
    return torch.from_numpy(np.array(x, order="C")).cuda()        # (a copy: the shared streams are read-only)


def run_direct(xd, N, mode, corr_in=None):
    c, m = zc_v2.correlate_batched(xd, Z.ref_c(N), mode, corr_in=corr_in, want_corr=True, want_mag=True, method="direct")
    return c, m


def run_fft(xd, N, mode, M):
    """ofs_zc_correlate_fft with the block length M the test planned with (plans shared by the module)."""
    batch = _lib.as_batch(xd, batched=True)
    key = (N, batch.B, batch.nb, batch.T, M)
    if key not in _plans:
        _plans[key] = zc_v2.MFPlan(Z.ref_c(N), batch.B, batch.nb, batch.T, batch.data.device, M=M)
    nout = batch.T + N - 1
    shape = (batch.B, batch.nb, nout) if mode == Z.RAW else (batch.B, nout)
    c = torch.empty(shape, dtype=torch.complex128, device=xd.device)
    m = torch.empty(shape, dtype=torch.float64, device=xd.device)
    _plans[key].run(batch, Z.ref_energy(N), mode, c, m)
    return c, m


def groups(n_big_only=False, small_only=False):
    """The cases grouped into launches: every family of one (N, T) is one batch."""
    out = {}
    for fam, N, T in Z.cases():
        if (n_big_only and N != Z.N_BIG) or (small_only and N == Z.N_BIG):
            continue
        out.setdefault((N, T), []).append(Z.stream(fam, N, T))
    return out


@pytest.mark.parametrize("fmt", ["int16", "c64", "c128"])
def test_direct_kernel_exact_on_integer_streams(fmt):
    worst = {}
    for (N, T), sts in groups().items():
        for nb in (1, 2, 3):
            xd = to_dev(np.stack([s.x(nb, fmt) for s in sts]))
            for mode in MODES + (Z.NORMALIZE,):
                ci = None
                if mode == Z.NORMALIZE:
                    if nb != 1:
                        continue
                    ci = np.stack([(lambda e: (e.re + 1j * e.im).astype(np.complex128)[0])(Z.expected(s, 1, Z.SUM)) for s in sts])
                c, m = run_direct(xd, N, mode, ci)
                c, m = c.cpu().numpy(), m.cpu().numpy()
                for i, s in enumerate(sts):
                    v = Z.check(s, nb, mode, c[i], m[i], "direct")
                    assert v, (s.name, nb, Z.MODE_NAME[mode], v.why)
                    assert v.n_checked == 2 * (nb if mode == Z.RAW else 1) * s.nout
                    if mode not in (Z.RAW, Z.SUM):
                        key = (Z.MODE_NAME[mode] if mode != Z.NORMALIZE else "normalize", nb)
                        # one branch: ulps of the exact value; more: of the bound (branch terms may cancel)
                        worst[key] = max(worst.get(key, 0.0), v.ulps if nb == 1 else v.ratio)
                        if "zero" in s.name:                   # all-zero windows: exactly +0.0
                            a, b = Z.zero_span(N, T)
                            z = c[i].reshape(-1)[a + N - 1:b]
                            assert z.size == Z.ZERO_EXTRA + 1 and not z.view(np.uint64).any(), (s.name, mode)
                            assert not m[i].reshape(-1)[a + N - 1:b].view(np.uint64).any()
    print(f"direct {fmt}: largest component error, one branch in ulps of the exact value (k = 5, COMBINED 6), "
          f"more branches as a fraction of the bound: {worst}")


def test_direct_kernel_takes_the_reference_side_of_the_clamp():
    st = Z.stream("straddle", 2048, 10243)
    cr, ci, e = st.exact()
    for nb in (1, 2, 3):
        xd = to_dev(st.x(nb, "c128")[None])
        for mode in MODES + ((Z.NORMALIZE,) if nb == 1 else ()):
            cin = (lambda ex: (ex.re + 1j * ex.im).astype(np.complex128))(Z.expected(st, 1, Z.SUM)) if mode == Z.NORMALIZE else None
            c, m = run_direct(xd, 2048, mode, cin)
            v = Z.check(st, nb, mode, c.cpu().numpy()[0], m.cpu().numpy()[0], "direct")
            assert v, (nb, Z.MODE_NAME[mode], v.why)
    # the two sides are told apart: at Σk² = 4 the clamp 1e-12 divides, at 5 the energy itself
    ex = Z.expected(st, 1, Z.V2)
    rn = np.sqrt(Z.LD(Z.ref_energy(2048)))
    for k, w in ((4, 1 / (rn * np.sqrt(Z.LD(1e-12)))), (5, 1 / (rn * np.sqrt(Z.LD(5) * Z.LD(2.0) ** -42)))):
        sel = (e[0] == k) & ((cr[0] != 0) | (ci[0] != 0))
        assert sel.any() and np.array_equal(ex.w[0, 0][sel], np.full(int(sel.sum()), w))


@pytest.mark.parametrize("fmt", ["int16", "c64", "c128"])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_overlap_save_within_the_per_block_bound(kernel, fmt, variant):
    for name, val in KERNELS[kernel].items():
        variant(name, val)
    worst, worst_blk = {}, 0.0
    sets = [(groups(n_big_only=True), (1, 2), kernel)]
    if kernel == "rocfft":
        sets.append((groups(small_only=True), (1, 2, 3), "rocfft"))      # 2048-point blocks: mc_extract_kernel
    if fmt == "c128":
        sets.append(({(2048, 10243): [Z.stream("straddle", 2048, 10243)]}, (1, 2), kernel))
    for grp, nbs, kern in sets:
        for (N, T), sts in grp.items():
            for nb in nbs:
                M = Z.pick_m(N, T, nb)
                xd = to_dev(np.stack([s.x(nb, fmt) for s in sts]))
                for mode in MODES:
                    c, m = run_fft(xd, N, mode, M)
                    c, m = c.cpu().numpy(), m.cpu().numpy()
                    for i, s in enumerate(sts):
                        v = Z.check(s, nb, mode, c[i], m[i], kern, M)
                        assert v, (kernel, s.name, nb, Z.MODE_NAME[mode], v.why)
                        assert v.n_checked == 2 * (nb if mode == Z.RAW else 1) * s.nout
                        assert (v.block_ratio <= 1).all() and v.block_ratio.size == -(-s.nout // (M - N + 1))
                        worst[Z.MODE_NAME[mode]] = max(worst.get(Z.MODE_NAME[mode], 0.0), v.ratio)
                        worst_blk = max(worst_blk, float(v.block_ratio.max()))
    K = EM.zc_os_K(Z.ref_c(2048), 8192, kernel)
    print(f"overlap-save {kernel} {fmt}: worst block |d corr| / bound {worst_blk:.3g} (K = {K:.0f}: "
          f"{worst_blk * K:.3g} of u·L·|u_q|·|ref|); worst ratio per mode, |corr| included: "
          + ", ".join(f"{k} {r:.3g}" for k, r in worst.items()))


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_inexact_energy_prefix_within_the_block_energy_model(kernel, variant):
    """2^27 next to 1 in one block: the overlap-save energy prefix is no longer exact, the window energy is
    held to |d e| <= ZC_OS_KE·u·E_block (so the quiet windows of that block are hardly constrained, as the
    header of zc_fftcorr.hip says); the direct kernel's corr is still the exact integers."""
    st = Z.stream("inexact", 2048, 16384)
    for name, val in KERNELS[kernel].items():
        variant(name, val)
    for nb in (1, 2):
        xd = to_dev(st.x(nb, "c128")[None])
        for mode in MODES:
            c, m = run_fft(xd, 2048, mode, Z.M_BIG)
            v = Z.check(st, nb, mode, c.cpu().numpy()[0], m.cpu().numpy()[0], kernel, Z.M_BIG, ke=EM.ZC_OS_KE)
            assert v, (kernel, nb, Z.MODE_NAME[mode], v.why)
            print(f"inexact {kernel} nb {nb} {Z.MODE_NAME[mode]}: worst ratio {v.ratio:.3g}")
            if kernel == "pers" and mode in (Z.RAW, Z.SUM):
                c, m = run_direct(xd, 2048, mode)
                v = Z.check(st, nb, mode, c.cpu().numpy()[0], m.cpu().numpy()[0], "direct")
                assert v, ("direct", nb, Z.MODE_NAME[mode], v.why)


def test_many_block_batch_on_the_persistent_kernel():
    """180 streams x 3 blocks: more blocks than compute units, runs of unequal length that cross stream
    boundaries; every stream is a delayed, rotated base stream, its expectation the base's shifted and
    rotated (exact).  Every output of every stream, V2 and RAW."""
    xd = to_dev(Z.batch_x())
    for mode in (Z.V2, Z.RAW):
        c, m = run_fft(xd, 2048, mode, Z.M_BIG)
        c, m = c.cpu().numpy(), m.cpu().numpy()
        worst = 0.0
        for b in range(Z.BATCH_B):
            v = Z.check(Z.batch_stream(b), 1, mode, c[b], m[b], "pers", Z.M_BIG, exp=Z.batch_expected(b, mode))
            assert v, (b, Z.batch_plan()[b], Z.MODE_NAME[mode], v.why)
            worst = max(worst, v.ratio)
        print(f"many-block batch {Z.MODE_NAME[mode]}: worst ratio {worst:.3g}")


def _bits(t):
    return torch.view_as_real(t).view(torch.int64) if t.is_complex() else t.view(torch.int64)


NF_STREAM = 77


@pytest.mark.parametrize("what,pos", [("nan", 5000), ("inf", 11000), ("-inf", 7000)])
def test_non_finite_sample_is_contained(what, pos, variant):
    """One non-finite sample in stream 77 of the many-block batch.  Direct kernel: the non-finite outputs are
    exactly those whose window holds it, every other word equals the clean run's.  Overlap-save kernels: a
    superset of those, inside the blocks whose input span holds it (5000: blocks 0 and 1; 11000: 1 and 2;
    7000: 1); every output of every other block and of every other stream equals the same kernel's clean run."""
    N, M, S = 2048, Z.M_BIG, Z.S_BIG
    x = Z.batch_x().copy()
    x[NF_STREAM, 0, pos] = {"nan": complex(np.nan, 1.0), "inf": complex(np.inf, 1.0), "-inf": complex(2.0, -np.inf)}[what]
    xc, xb = to_dev(Z.batch_x()), to_dev(x)
    nout = Z.BATCH_T + N - 1
    win = torch.zeros(nout, dtype=torch.bool, device="cuda")
    win[pos:pos + N] = True
    blocks = Z.blocks_holding(pos, N, M, nout)
    assert blocks == {5000: [0, 1], 11000: [1, 2], 7000: [1]}[pos]
    blk = torch.zeros(nout, dtype=torch.bool, device="cuda")
    for q in blocks:
        blk[q * S:(q + 1) * S] = True
    others = torch.ones(Z.BATCH_B, dtype=torch.bool, device="cuda")
    others[NF_STREAM] = False
    for kernel in ("direct",) + tuple(KERNELS):
        for name, val in KERNELS.get(kernel, {}).items():
            variant(name, val)
        for mode in (Z.RAW, Z.V2):
            run = (lambda z: run_direct(z, N, mode)) if kernel == "direct" else (lambda z: run_fft(z, N, mode, M))
            (c0, m0), (c1, m1) = run(xc), run(xb)
            c0, c1, m0, m1 = (t.reshape(Z.BATCH_B, nout) for t in (c0, c1, m0, m1))
            assert torch.isfinite(torch.view_as_real(c0)).all() and torch.isfinite(m0).all()
            assert torch.equal(_bits(c0[others]), _bits(c1[others])) and torch.equal(_bits(m0[others]), _bits(m1[others])), \
                (kernel, mode, "another stream changed")
            bad_c = ~torch.isfinite(torch.view_as_real(c1[NF_STREAM])).all(dim=-1)
            bad_m = ~torch.isfinite(m1[NF_STREAM])
            keep = ~win if kernel == "direct" else ~blk
            assert torch.equal(_bits(c0[NF_STREAM][keep]), _bits(c1[NF_STREAM][keep])), (kernel, mode)
            assert torch.equal(_bits(m0[NF_STREAM][keep]), _bits(m1[NF_STREAM][keep])), (kernel, mode)
            if kernel == "direct":
                assert torch.equal(bad_c, win) and torch.equal(bad_m, win), (kernel, mode)
            else:
                assert (bad_c >= win).all() and (bad_m >= win).all() and not (bad_c & ~blk).any() and not (bad_m & ~blk).any()
        _lib.reset_variants()


@pytest.mark.parametrize("kernel", ["direct"] + list(KERNELS))
def test_huge_samples_stay_finite_and_overflowing_windows_give_zero(kernel, variant):
    """noise·2^654 (c128): |corr| up to 9e199 is exact in the direct kernel and inside the per-block bound in
    the overlap-save kernels, |corr| finite and within the counted ulps of the exact root (sqrt(re² + im²)
    overflows for |c| > 1.3e154); every window's energy overflows to +inf while corr stays finite, so every
    normalised output is 0, as corr / (ref_norm·sqrt(inf)) is in zc_v2.py:269-271."""
    st = Z.stream("huge", 2048, 16384)
    assert float(np.max(Z.expected(st, 1, Z.RAW).mag)) > 5e199
    e = st.exact()[2]
    assert (e[:, :st.nout] > 0).all()                          # every window holds a sample: its energy overflows
    for name, val in KERNELS.get(kernel, {}).items():
        variant(name, val)
    for nb in (1, 2):
        xd = to_dev(st.x(nb, "c128")[None])
        for mode in MODES:
            c, m = run_direct(xd, 2048, mode) if kernel == "direct" else run_fft(xd, 2048, mode, Z.M_BIG)
            c, m = c.cpu().numpy()[0], m.cpu().numpy()[0]
            if mode in (Z.RAW, Z.SUM):
                v = Z.check(st, nb, mode, c, m, kernel, Z.M_BIG)
                assert v, (kernel, nb, Z.MODE_NAME[mode], v.why)
                print(f"huge {kernel} nb {nb} {Z.MODE_NAME[mode]}: worst ratio {v.ratio:.3g}, largest |corr| {m.max():.3g}")
            else:
                assert np.isfinite(c.real).all() and np.isfinite(c.imag).all(), (kernel, nb, Z.MODE_NAME[mode])
                assert (c == 0).all() and (m == 0).all() and not np.signbit(m).any(), (kernel, nb, Z.MODE_NAME[mode])
