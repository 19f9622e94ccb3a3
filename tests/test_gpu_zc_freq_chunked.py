"""Resumable chunked zc_freq metric with a running peak (csrc/zc_freq_chunk.hip, csrc/zs_body.h,
zc_freq.FrequencyMetricChunked, ofs_zc_freq_metric_chunk).

The yardstick of every case is ONE one-shot batched call on the whole stream (ofs_zc_freq_metric on its
sliding kernel, the same format and precision; every case first asserts more than 64 offsets, so that
the complex64 one-shot call is plan 5 and not the fp32 window FFT).  Any chunking must reproduce it BIT
FOR BIT: the metric concatenated over the pushes, its first N + cp - 1 elements (offsets s < 0, all-zero
bits) dropped, is the [T - (N+cp) + 1] array of the one-shot call.  Every comparison is ``torch.equal``
on integer bit views (a NaN equals the same NaN, +0.0 differs from -0.0): no tolerance anywhere.  The one
thing left out, in test_nan_sample alone, is the sign bit of a word that is NaN in the one-shot result.
The running peak is checked after EVERY push against np.argmax (= ofs_row_argmax, checked once per case)
of the one-shot metric truncated to the offsets seen so far.  So that the pair is not equal and wrong,
test_templates also holds both against the CPU oracle at the sliding kernel's own bound
(tests/test_gpu_corr.py: rtol 1e-9 + atol 1e-11; rtol 2^-22 for the float32 result).
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import ofdm_oracle as O
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ofdm_sync_amd import _lib, zc_freq  # noqa: E402

FMTS = {"c64": _lib.C64, "c128": _lib.C128, "i16": _lib.CI16}


def _C(N):
    """Chunk length of the sliding kernel (csrc/zs_body.h zs_chunk_len)."""
    return 256 if N >= 8192 and N % 256 == 0 else 128 if N % 128 == 0 else 64


# ------------------------------------------------------------------------------------------
# inputs, the one-shot yardstick, comparison
# ------------------------------------------------------------------------------------------
def _to_dev(x, fmt):
    """complex host array [B, nb, T] -> device tensor of the format (int16: values rounded, I/Q last)."""
    if fmt == "i16":
        return torch.from_numpy(np.stack([np.round(x.real), np.round(x.imag)], -1).astype(np.int16)).cuda()
    return torch.from_numpy(x.astype(np.complex64 if fmt == "c64" else np.complex128)).cuda()


def _host(xd):
    """The samples a device tensor holds, as complex128 [B, nb, T]."""
    a = xd.cpu().numpy()
    return a[..., 0] + 1j * a[..., 1] if a.dtype == np.int16 else a.astype(np.complex128)


@functools.lru_cache(maxsize=None)
def _stream(fmt, nb, B, T, N, seed=0):
    """Seeded noise with a PSS symbol in stream 0 (int16: scaled to +-2000); the last stream has a 60 dB
    loud -> quiet step in its middle.  Computed once per shape, left unchanged."""
    rng = np.random.default_rng(1000 * T + 10 * nb + B + 7919 * seed)
    x = (rng.standard_normal((B, nb, T)) + 1j * rng.standard_normal((B, nb, T))) / np.sqrt(2.0)
    if T >= N + 40:
        x[0, :, 37:37 + N] += 3 * O.pss_symbol(N)
    x[B - 1, :, T // 2:] *= 1e-3
    return _to_dev(x * 500 if fmt == "i16" else x, fmt)


def _template():
    """The PSS template (bins +-1 .. +-31: mirror pairs, so the pair body runs)."""
    idx, t, e = O.zc_template()
    return np.asarray(idx), np.asarray(t), float(e)


def _one_shot(xd, N, cp, tmpl):
    nb_T = xd.shape[2]
    assert nb_T - (N + cp) + 1 > 64, "the complex64 one-shot call must be the sliding kernel (plan 5)"
    fmt = {torch.complex64: "c64", torch.complex128: "c128", torch.int16: "i16"}[xd.dtype]
    prec = _lib.FP32 if fmt == "c64" else _lib.FP64
    assert _lib.lib().ofs_zc_freq_plan(FMTS[fmt], prec, nb_T, N, cp) == (5 if fmt == "c64" else 4)
    m = zc_freq.compute_frequency_metric_batched(xd, *tmpl, N=N, cp=cp)
    assert m.dtype == (torch.float32 if fmt == "c64" else torch.float64)
    assert m.shape == (xd.shape[0], nb_T - (N + cp) + 1)
    return m


@functools.lru_cache(maxsize=None)
def _ref(fmt, nb, B, T, N, cp, seed=0):
    """The one-shot call on the whole cached stream with the PSS template (once per input, unchanged)."""
    return _one_shot(_stream(fmt, nb, B, T, N, seed), N, cp, _template())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _det(xd, N, cp, tmpl=None):
    B, nb = xd.shape[0], xd.shape[1]
    kw = {} if tmpl is None else dict(bin_indices=tmpl[0], template_bins=tmpl[1], template_energy=tmpl[2])
    return zc_freq.FrequencyMetricChunked(B, nb, dtype=xd.dtype, N=N, cp=cp, **kw)


class Push:
    """Clones of one push's outputs, enqueued on the same stream (the object reuses its buffers)."""

    def __init__(self, det, m, n_after):
        self.m = None if m is None else m.clone()
        self.off0, self.pi, self.pv = det.off0.clone(), det.peak_index.clone(), det.peak_value.clone()
        self.n_after = n_after


def _feed(det, xd, cuts, final=True, n0=0):
    """Push xd[:, :, a:b] for consecutive cut points back to back, without any host synchronisation."""
    out, s, n = [], 0, n0
    assert sum(cuts) == xd.shape[2] and all(c > 0 for c in cuts), (cuts, xd.shape)
    for i, c in enumerate(cuts):
        m = det.push(xd[:, :, s:s + c].contiguous(), final=final and i == len(cuts) - 1)
        assert m.shape == (xd.shape[0], c)
        s, n = s + c, n + c
        out.append(Push(det, m, n))
    return out


def _check(res, ref, N, cp, what="", rows=None, nan_sign_free=False, n0=0):
    """Concatenated metric: all-zero bits for s < 0, then the one-shot array bit for bit; off0 of every
    push; the peak after every push = first argmax of the one-shot metric over the offsets so far."""
    need = N + cp
    got = _bits(torch.cat([r.m for r in res], dim=1))
    want = _bits(ref)
    sel = list(range(want.shape[0])) if rows is None else list(rows)
    fill = max(need - 1 - n0, 0)
    skip = max(n0 - (need - 1), 0)                       # offsets before the first push
    assert got.shape[1] - fill == want.shape[1] - skip, (what, got.shape, want.shape)
    assert not bool(got[sel][:, :fill].any()), (what, "fill phase is not +0.0")
    got, want = got[:, fill:], want[:, skip:]
    if nan_sign_free:
        nan = torch.isnan(ref[:, skip:])
        mask = 0x7fffffff if got.dtype == torch.int32 else 0x7fffffffffffffff
        got, want = torch.where(nan, got & mask, got), torch.where(nan, want & mask, want)
    if not torch.equal(got[sel], want[sel]):
        bad = (got[sel] != want[sel]).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} words differ from the one-shot call, first at {bad[0].tolist()}")
    refh = ref.double().cpu().numpy()
    n = n0
    for r in res:
        off0, pi, pv = r.off0.cpu().numpy(), r.pi.cpu().numpy(), r.pv.cpu().numpy()
        k = r.n_after - need + 1                         # offsets the stream has after this push
        for b in sel:
            assert off0[b] == n - need + 1, (what, b, off0[b], n)
            if k <= 0:
                assert pi[b] == -1 and pv[b] == 0.0 and not np.signbit(pv[b]), (what, b, pi[b], pv[b])
                continue
            i = int(np.argmax(refh[b, :k]))
            assert pi[b] == i, (what, "peak_index", b, r.n_after, pi[b], i)
            assert pv[b] == refh[b, i] or (np.isnan(pv[b]) and np.isnan(refh[b, i])), (what, "peak_value", b)
        n = r.n_after
    return got


def _splits(T, N, cp, one_sample):
    """The chunkings of the issue for a stream of T samples."""
    need, C, Hr = N + cp, _C(N), N + _C(N)
    rng = np.random.default_rng(T + N + cp)
    out = {"one push": [T]}
    if one_sample:
        out["1-sample pushes"] = [1] * T
    # pushes that end exactly at, one before and one after every multiple of C in offset space: the next
    # push's first offset n - need + 1 is kC - 1, kC, kC + 1
    ends = sorted({need - 1 + k * C + d for k in range(0, T // C + 2) for d in (-1, 0, 1)} & set(range(1, T)))
    out["around every multiple of C"] = np.diff([0] + ends + [T]).tolist()
    big = Hr + 7                                         # longer than the ring, then shorter ones
    assert big < T
    rest = T - big
    out["longer than the ring, then short"] = [big] + [50] * (rest // 50) + ([rest % 50] if rest % 50 else [])
    first = need - 3                                     # the whole first call is in the fill phase
    out["first push all fill"] = [first, (T - first) // 2, T - first - (T - first) // 2]
    for i in range(3):
        k = int(rng.integers(2, 9))
        cuts = np.sort(rng.choice(np.arange(1, T), size=k, replace=False))
        out[f"random {i}"] = np.diff(np.concatenate(([0], cuts, [T]))).tolist()
    return out


# ------------------------------------------------------------------------------------------
# Case 1: bit equality under chunking
# ------------------------------------------------------------------------------------------
SHAPES = [(64, 0), (128, 9), (192, 16), (256, 64), (2048, 512)]


@pytest.mark.parametrize("N,cp", SHAPES)
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("fmt", ["c64", "c128", "i16"])
def test_any_chunking_equals_one_shot(fmt, nb, N, cp):
    B, T = 3, N + cp + 3 * _C(N) + 5
    xd, ref = _stream(fmt, nb, B, T, N), _ref(fmt, nb, B, T, N, cp)
    assert zc_freq.peak_index_batched(ref)[0].cpu().tolist() == np.argmax(ref.cpu().numpy(), axis=1).tolist()
    for name, cuts in _splits(T, N, cp, one_sample=N <= 192).items():
        _check(_feed(_det(xd, N, cp), xd, cuts), ref, N, cp, what=f"{fmt} nb={nb} N={N} cp={cp} {name}")


def test_any_chunking_equals_one_shot_n8192():
    """C = 256 (N >= 8192): complex128, one branch, two streams."""
    N, cp, B = 8192, 0, 2
    T = N + cp + 3 * 256 + 5
    xd, ref = _stream("c128", 1, B, T, N), _ref("c128", 1, B, T, N, cp)
    for name, cuts in _splits(T, N, cp, one_sample=False).items():
        _check(_feed(_det(xd, N, cp), xd, cuts), ref, N, cp, what=f"N=8192 {name}")


@pytest.mark.parametrize("nb,defer,N", [(2, 1, 4096), (2, 1, 2048), (1, 0, 256), (2, 0, 256)])
def test_row_sum_variant_selects_both_calls_alike(nb, defer, N):
    """ZS_DEFER forces the deferred (LDS) or the per-step DPP row sums, which differ in the last bits: both
    calls must take the same form whatever their W.  Two branches on the pair body defer only where
    every W fits the block region, N/C >= 18 (N = 4096), and fall back to DPP below (N = 2048) - by a
    rule free of the offset count, so the chunked call, whose workgroups are smaller, still agrees."""
    cp, B = 0, 2
    T = N + cp + 3 * _C(N) + 5
    xd = _stream("c128", nb, B, T, N, seed=2)
    with _lib.variants(ZS_DEFER=defer):
        ref = _one_shot(xd, N, cp, _template())
        for name in ("one push", "around every multiple of C", "random 0"):
            _check(_feed(_det(xd, N, cp), xd, _splits(T, N, cp, False)[name]), ref, N, cp,
                   what=f"ZS_DEFER={defer} nb={nb} N={N} {name}")


@pytest.mark.parametrize("fmt,nb,N,cp", [("c64", 2, 128, 9), ("c128", 1, 192, 16), ("i16", 2, 64, 0)])
def test_push_without_metric_still_advances_the_ring(fmt, nb, N, cp):
    """A want_metric=False push takes the samples in: the next pushes' outputs are the one-shot call's;
    the peak, which needs the metric, does not advance in it."""
    B, T = 3, N + cp + 3 * _C(N) + 5
    xd, ref = _stream(fmt, nb, B, T, N), _ref(fmt, nb, B, T, N, cp)
    det = _det(xd, N, cp)
    a, b = N + cp + 11, N + cp + 11 + _C(N) + 3
    head = _feed(det, xd[:, :, :a], [a - 20, 20], final=False)
    before = (det.peak_index.clone(), det.peak_value.clone())
    assert det.push(xd[:, :, a:b].contiguous(), want_metric=False) is None
    assert det.n_seen == b
    assert torch.equal(det.peak_index, before[0]) and torch.equal(det.peak_value, before[1])
    assert det.off0.cpu().tolist() == [a - (N + cp) + 1] * B
    tail = det.push(xd[:, :, b:].contiguous(), final=True)
    got = _bits(torch.cat([r.m for r in head] + [tail], dim=1))
    want = _bits(ref)
    fill = N + cp - 1
    assert not bool(got[:, :fill].any())
    assert torch.equal(got[:, fill:a], want[:, :a - fill])
    assert torch.equal(got[:, a:], want[:, b - fill:])
    assert det.off0.cpu().tolist() == [b - (N + cp) + 1] * B


# ------------------------------------------------------------------------------------------
# Case 2: the one-shot call's workgroup-group edge
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb,edge", [(1, 8 * 16 * 128), (2, 4 * 8 * 128)])
def test_workgroup_group_edge(nb, edge):
    """N = 128: the one-shot call takes two workgroups per stream from `edge` offsets on (chunks per wave x
    waves x C); the pushes' own workgroups begin elsewhere and must not matter."""
    N, cp, B = 128, 0, 2
    T = N + cp + edge + 300
    xd, ref = _stream("c128", nb, B, T, N), _ref("c128", nb, B, T, N, cp)
    assert ref.shape[1] > edge
    cuts = [1000] * (T // 1000) + ([T % 1000] if T % 1000 else [])
    _check(_feed(_det(xd, N, cp), xd, cuts), ref, N, cp, what=f"group edge nb={nb}")


# ------------------------------------------------------------------------------------------
# Case 3: templates on both bodies, against the one-shot call and the CPU oracle
# ------------------------------------------------------------------------------------------
def _tmpl(name, rng):
    idx, t, e = _template()
    if name == "pss_shuffled":                            # pair body
        perm = rng.permutation(idx.size)
        idx, t = idx[perm], t[perm]
    elif name == "one_pair":                              # pair body
        idx, t = np.array([-7, 7]), np.array([1.0 + 0.5j, -0.25 + 1j])
    elif name == "unpaired":                              # per-bin body
        idx = np.arange(1, 40)
        t = rng.standard_normal(idx.size) + 1j * rng.standard_normal(idx.size)
    elif name == "with_dc_and_nyquist":                   # per-bin body: bins 0 and N/2
        idx = np.concatenate((np.arange(-20, 21), [128]))
        t = rng.standard_normal(idx.size) + 1j * rng.standard_normal(idx.size)
    return idx, t, float(np.sum(np.abs(t) ** 2))


@pytest.mark.parametrize("fmt,nb", [("c128", 1), ("c128", 2), ("c64", 1), ("i16", 2)])
@pytest.mark.parametrize("name", ["pss_shuffled", "one_pair", "unpaired", "with_dc_and_nyquist"])
def test_templates(name, fmt, nb):
    N, cp, B = 256, 64, 2
    T = N + cp + 3 * _C(N) + 5
    rng = np.random.default_rng(len(name) * 131 + nb)
    tmpl = _tmpl(name, rng)
    xd = _stream(fmt, nb, B, T, N, seed=3)
    ref = _one_shot(xd, N, cp, tmpl)
    xh = _host(xd)
    for b in range(B):                                    # the yardstick itself is right (the kernel's own bound)
        mo = O.zc_freq_metric(xh[b], N, cp, *tmpl)
        if fmt == "c64":
            np.testing.assert_allclose(ref[b].cpu().numpy().astype(np.float64), mo, rtol=2.0 ** -22, atol=1e-12)
        else:
            np.testing.assert_allclose(ref[b].cpu().numpy(), mo, rtol=1e-9, atol=1e-11)
    splits = _splits(T, N, cp, one_sample=False)
    for key in ("one push", "around every multiple of C", "random 0", "random 1"):
        got = _check(_feed(_det(xd, N, cp, tmpl), xd, splits[key]), ref, N, cp, what=f"{name} {fmt} nb={nb} {key}")
    gh = got.view(ref.dtype).cpu().numpy().astype(np.float64)
    for b in range(B):                                    # and so is the chunked result
        mo = O.zc_freq_metric(xh[b], N, cp, *tmpl)
        np.testing.assert_allclose(gh[b], mo, rtol=2.0 ** -22 if fmt == "c64" else 1e-9,
                                   atol=1e-12 if fmt == "c64" else 1e-11)


# ------------------------------------------------------------------------------------------
# Case 4: the running peak
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zcfreq_N2048", "zcfreq_N256"])
def test_peak_on_reference_goldens(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    N, cp = int(d["N"]), int(d["CP"])
    x = np.asarray(d["x"], np.complex128)
    x = x[None, None, :] if x.ndim == 1 else x[None]
    T = x.shape[2]
    assert T - (N + cp) + 1 > 64
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    det = zc_freq.FrequencyMetricChunked(1, x.shape[1], dtype=torch.complex128, N=N, cp=cp)
    cuts = [N // 2 + 7] * (T // (N // 2 + 7)) + ([T % (N // 2 + 7)] if T % (N // 2 + 7) else [])
    res = _feed(det, xd, cuts)
    assert int(res[-1].pi[0]) == int(np.argmax(d["metric"]))
    m = torch.cat([r.m for r in res], dim=1)[0, N + cp - 1:].cpu().numpy()
    np.testing.assert_allclose(m, d["metric"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(float(res[-1].pv[0]), np.max(d["metric"]), rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("fmt,nb,N,P", [("c128", 1, 64, 128), ("i16", 2, 128, 128), ("c64", 1, 192, 64)])
def test_peak_exact_ties_report_the_first(fmt, nb, N, P):
    """A stream that repeats with a period P that is a multiple of C: outputs one period apart read equal
    samples at the same place of their chunks, so they are bit-equal and the maximum occurs at least
    twice.  The peak is the first (np.argmax)."""
    cp, B = 0, 2
    assert P % _C(N) == 0
    T = N + cp + 2 * P + 70
    rng = np.random.default_rng(N + P)
    per = (rng.standard_normal((B, nb, P)) + 1j * rng.standard_normal((B, nb, P))) * 300
    x = np.tile(per, (1, 1, T // P + 1))[:, :, :T]
    xd = _to_dev(x, fmt)
    xh = _host(xd)
    tmpl = _template()
    ref = _one_shot(xd, N, cp, tmpl)
    refh = ref.cpu().numpy()
    for b in range(B):                                    # the tie exists in the reference arithmetic too
        mo = O.zc_freq_metric(xh[b], N, cp, *tmpl)
        i = int(np.argmax(mo))
        assert i < P and mo[i] == mo[i + P]
        j = int(np.argmax(refh[b]))
        assert j < P and refh[b, j] == refh[b, j + P] and (refh[b] == refh[b, j]).sum() >= 2
    splits = _splits(T, N, cp, one_sample=False)
    for key in ("one push", "around every multiple of C", "random 0"):
        res = _feed(_det(xd, N, cp), xd, splits[key])
        _check(res, ref, N, cp, what=f"ties {fmt} {key}")
        assert res[-1].pi.cpu().tolist() == [int(np.argmax(refh[b])) for b in range(B)]


@pytest.mark.parametrize("fmt,nb", [("c128", 1), ("c64", 2)])
def test_nan_sample(fmt, nb):
    """One NaN sample: the metric is NaN exactly where the one-shot call's is (sign bit masked), bit-equal
    again after the affected chunk, and the peak is the first NaN offset from the push that brings it."""
    N, cp, B = 128, 9, 3
    C = _C(N)
    T = N + cp + 5 * C + 5
    x = _host(_stream(fmt, nb, B, T, N, seed=5)).copy()
    p = N + cp + C + 40                                    # inside the stream: offsets p - N - cp + 1 .. p - cp
    x[1, nb - 1, p] = complex(np.nan, 1.0)
    xd = _to_dev(x, fmt)
    ref = _one_shot(xd, N, cp, _template())
    nan = torch.isnan(ref).cpu().numpy()
    first = p - (N + cp) + 1
    assert not nan[0].any() and not nan[2].any() and nan[1].any()
    assert int(np.flatnonzero(nan[1])[0]) == first
    last = int(np.flatnonzero(nan[1])[-1])
    assert last < ref.shape[1] - 1, "outputs after the affected chunks are numbers again"
    assert (last + 1) % C == 0                             # the NaN stays in the recursion to its chunk's end
    splits = _splits(T, N, cp, one_sample=False)
    for key in ("one push", "around every multiple of C", "random 0", "random 2"):
        res = _feed(_det(xd, N, cp), xd, splits[key])
        got = _check(res, ref, N, cp, what=f"nan {fmt} {key}", nan_sign_free=True)
        assert torch.equal(got[:, last + 1:], _bits(ref)[:, last + 1:])
        assert int(res[-1].pi[1]) == first and bool(torch.isnan(res[-1].pv[1]))
        for r in res:
            assert int(r.pi[1]) == first if r.n_after > p else int(r.pi[1]) != first


def test_peak_is_empty_while_filling():
    N, cp, B = 128, 9, 2
    T = N + cp + 3 * _C(N) + 5
    xd = _stream("c128", 1, B, T, N)
    det = _det(xd, N, cp)
    for a, b in ((0, 50), (50, N + cp - 1)):
        m = det.push(xd[:, :, a:b].contiguous())
        assert not bool(_bits(m).any())
        assert det.peak_index.cpu().tolist() == [-1] * B and _bits(det.peak_value).cpu().tolist() == [0] * B
        assert det.off0.cpu().tolist() == [a - (N + cp) + 1] * B
    det.push(xd[:, :, N + cp - 1:N + cp].contiguous())      # the first window is complete
    assert det.peak_index.cpu().tolist() == [0] * B
    assert torch.equal(det.peak_value, _ref("c128", 1, B, T, N, cp)[:, 0])


# ------------------------------------------------------------------------------------------
# Case 5: state handling
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,nb", [("c64", 1), ("i16", 2)])
def test_final_and_flush_leave_fresh_streams(fmt, nb):
    N, cp, B = 192, 16, 3
    T = N + cp + 3 * _C(N) + 5
    xd, ref = _stream(fmt, nb, B, T, N), _ref(fmt, nb, B, T, N, cp)
    cuts = _splits(T, N, cp, False)["random 1"]
    fresh = _feed(_det(xd, N, cp), xd, cuts)
    det = _det(xd, N, cp)
    other = _stream(fmt, nb, B, T, N, seed=9)
    _feed(det, other, [T - 100, 100], final=True)          # final on the last push
    assert det.n_seen == 0 and not bool(det.state[:, :64].any())
    again = _feed(det, xd, cuts, final=False)
    _check(again, ref, N, cp, what="after final")
    for r, q in zip(again, fresh):
        assert torch.equal(_bits(r.m), _bits(q.m)) and torch.equal(r.pi, q.pi) and torch.equal(r.off0, q.off0)
    before = (det.peak_index.clone(), det.peak_value.clone())
    det.flush()                                            # flush: the outputs once more, then fresh
    assert torch.equal(det.peak_index, before[0]) and torch.equal(det.peak_value, before[1])
    assert det.off0.cpu().tolist() == [T - (N + cp) + 1] * B
    assert det.n_seen == 0 and not bool(det.state[:, :64].any())
    _check(_feed(det, xd, cuts), ref, N, cp, what="after flush")


def test_reset_of_one_row_in_mid_stream():
    """reset(rows=[1]) puts stream 1 at n = 0 while stream 0 goes on: both are right in the same calls."""
    fmt, nb, N, cp, B = "c128", 2, 128, 9, 2
    T = N + cp + 3 * _C(N) + 5
    xd, ref = _stream(fmt, nb, B, T, N), _ref(fmt, nb, B, T, N, cp)
    a = N + cp + 77
    det = _det(xd, N, cp)
    head = _feed(det, xd[:, :, :a], [a - 30, 30], final=False)
    det.reset(rows=[1])
    # stream 0 continues with its samples; stream 1 starts the same stream over
    k = T - a
    mix = torch.stack([xd[0, :, a:], xd[1, :, :k]]).contiguous()
    cuts = [k // 3, k - k // 3]
    tail = _feed(det, mix, cuts, final=False, n0=a)
    _check(head + tail, ref, N, cp, rows=[0], what="stream 0 goes on")
    # stream 1: a fresh stream of its first k samples (off0, fill phase and peak from n = 0)
    one = _feed(_det(xd, N, cp), xd[:, :, :k].contiguous(), cuts, final=False)
    for r, q in zip(tail, one):
        assert torch.equal(_bits(r.m[1]), _bits(q.m[1]))
        assert int(r.off0[1]) == int(q.off0[1]) and int(r.pi[1]) == int(q.pi[1])
        assert torch.equal(_bits(r.pv[1]), _bits(q.pv[1]))
    _check(one, ref[:, :k - (N + cp) + 1], N, cp, rows=[1], what="stream 1 from n = 0")


def test_shapes_the_size_function_refuses_raise():
    for kw in (dict(N=2000), dict(N=32), dict(N=2048, cp=-1)):
        with pytest.raises(ValueError):
            zc_freq.FrequencyMetricChunked(2, 1, dtype=torch.complex64, **kw)
    with pytest.raises(ValueError):
        zc_freq.FrequencyMetricChunked(2, 3, dtype=torch.complex64)
    with pytest.raises(ValueError):
        zc_freq.FrequencyMetricChunked(2, 1, dtype=torch.float32)
    det = zc_freq.FrequencyMetricChunked(2, 1, dtype=torch.complex64)       # the module's N_FFT / CYCLIC_PREFIX, PSS
    assert (det.N, det.cp) == (zc_freq.N_FFT, zc_freq.CYCLIC_PREFIX)
    with pytest.raises(ValueError):
        det.push(torch.zeros((2, 1, 0), dtype=torch.complex64, device="cuda"))


# ------------------------------------------------------------------------------------------
# Case 6: the premise - the one-shot call on a prefix is a prefix of the one-shot call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,nb,N,cp", [("c128", 1, 128, 9), ("c64", 2, 192, 16), ("i16", 1, 256, 64),
                                         ("c128", 2, 2048, 512)])
def test_one_shot_prefix_property(fmt, nb, N, cp):
    B, C = 3, _C(N)
    T = N + cp + 3 * C + 5
    xd, ref = _stream(fmt, nb, B, T, N), _ref(fmt, nb, B, T, N, cp)
    for Tp in (N + cp + 64, N + cp + C - 1 + 64, N + cp + 2 * C + 1, T - 1):
        m = _one_shot(xd[:, :, :Tp].contiguous(), N, cp, _template())
        assert torch.equal(_bits(m), _bits(ref[:, :Tp - (N + cp) + 1])), (fmt, nb, N, cp, Tp)
