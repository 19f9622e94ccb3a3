"""Resumable chunked S&C / combined S&C / Minn window metrics for complex64 streams (csrc/win_chunk.hip,
_metrics.WindowMetricChunked, ofs_win_metric_chunk).

The yardstick of every case is ONE one-shot batched call on the whole stream (ofs_sc_metric /
ofs_minn_metric, complex64, fp32) on its fast plan (ofs_win_plan > 0, asserted).  Any chunking must
reproduce it BIT FOR BIT: each output concatenated over the calls, its first N - 1 elements (d < 0,
all-zero bits) dropped, equals the [T - N + 1] array of the one-shot call.  Every comparison is
``torch.equal`` on int32 bit views (a NaN equals the same NaN, +0.0 differs from -0.0): no tolerance
anywhere against the one-shot call.  The one thing left out, in test_non_finite_samples alone, is the sign
bit of a word that is NaN in the one-shot result.  The fp32 arithmetic is not exact, so all this holds
only if a call continues the same fp32 partials, the same fp64 row scans and the same carried fp64 bases.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import error_models as EM
import ofdm_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from ofdm_sync_amd import _lib, _metrics, combined_sc_min, minn, sc, synth  # noqa: E402

KIND = {"sc": 1, "comb": 2, "minn": 3}
KEYS = ("M", "P", "R")
ORACLE = {"sc": O.sc_metric, "comb": O.comb_sc_metric, "minn": O.minn_metric}


def _N(kind, W):
    return 4 * W if kind == "minn" else 2 * W


# ------------------------------------------------------------------------------------------
# inputs, the one-shot yardstick, comparison
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stream(W, nb, B, T, seed=0):
    """complex64 [B, nb, T] on the GPU (synth.make_aa_batch / synth.synth_batch); the last stream has a
    60 dB loud -> quiet step in its middle.  Computed once per shape and left unchanged."""
    L = min(W, 1024)
    s = 7 * W + 3 * T + nb + 1000 * seed
    if nb == 1:
        x = synth.make_aa_batch(B, T, L, seed=s, device="cuda")
    else:
        x = synth.synth_batch(synth.faded_base(L, "cir1", (0, 1)), B, T, seed=s)
    assert x.shape == (B, nb, T) and x.dtype == torch.complex64
    x[B - 1, :, T // 2:] *= 1e-3
    return x


def _one_shot(kind, x, N):
    B, nb, T = x.shape
    assert _lib.lib().ofs_win_plan(KIND[kind], _lib.C64, _lib.FP32, nb, T, N) > 0, (kind, nb, T, N)
    if kind == "sc":
        out = sc.sc_streaming_metric_batched(x, N)
    elif kind == "comb":
        out = combined_sc_min.schmidl_cox_streaming_metric_batched(x, N)
    else:
        out = minn.minn_streaming_metric_batched(x, N)
    M, P, R = out
    assert M.dtype == torch.float32 and P.dtype == torch.complex64 and M.shape == (B, T - N + 1)
    return {"M": M, "P": P, "R": R}


@functools.lru_cache(maxsize=None)
def _ref(kind, W, nb, B, T, seed=0):
    """The one-shot call on the whole cached stream (computed once per input, left unchanged)."""
    return _one_shot(kind, _stream(W, nb, B, T, seed), _N(kind, W))


def _bits(t):
    if t.dtype == torch.complex64:
        return torch.view_as_real(t).contiguous().view(torch.int32)
    assert t.dtype == torch.float32, t.dtype
    return t.contiguous().view(torch.int32)


def _snap(r):
    """Clone of a push result, enqueued on the same stream (the object reuses its buffers)."""
    return _metrics.WindowChunkResult(*[None if t is None else t.clone() for t in (r.M, r.P, r.R, r.d0)])


def _cut(xt, chunks):
    out, s = [], 0
    for c in chunks:
        out.append(xt[:, :, s:s + c].contiguous())
        s += c
    assert s == xt.shape[2], (s, xt.shape)
    return out


def _feed(det, pieces, final=True, flush=False):
    """Push the pieces back to back without any host synchronisation."""
    res = [_snap(det.push(p, final=final and not flush and i == len(pieces) - 1)) for i, p in enumerate(pieces)]
    if flush:
        f = _snap(det.flush())
        assert f.M is None and f.P is None and f.R is None
        res.append(f)
    return res


def _assert_equal(res, ref, N, rows=None, what="", keys=KEYS, nan_sign_free=False):
    """Concatenated outputs: all-zero bits for d < 0, then the one-shot arrays bit for bit.
    nan_sign_free (test_non_finite_samples only): a word that is NaN in the one-shot result is compared
    without its sign bit - the NaN must be there, with the same payload."""
    body = [r for r in res if any(getattr(r, k) is not None for k in KEYS)]
    for k in keys:
        got = _bits(torch.cat([getattr(r, k) for r in body], dim=1))
        want = _bits(ref[k])
        sel = list(range(want.shape[0])) if rows is None else list(rows)
        assert got.shape[1] == want.shape[1] + N - 1, (what, k, got.shape, want.shape)
        assert not bool(got[sel][:, :N - 1].any()), (what, k, "fill phase is not +0.0")
        got = got[:, N - 1:]
        if nan_sign_free:
            w = ref[k]
            nan = torch.isnan(torch.view_as_real(w) if w.is_complex() else w)
            got = torch.where(nan, got & 0x7fffffff, got)
            want = torch.where(nan, want & 0x7fffffff, want)
        if not torch.equal(got[sel], want[sel]):
            bad = (got[sel] != want[sel]).nonzero()
            raise AssertionError((what, k, "first differing [row, index(, part)]", bad[0].tolist(), "of", len(bad)))


def _assert_d0(res, chunks, N, what=""):
    """d0 of call i = (samples of earlier calls) - (N - 1), for every stream."""
    seen = 0
    for r, c in zip(res, list(chunks) + [0]):
        assert r.d0.tolist() == [seen - (N - 1)] * r.d0.shape[0], (what, seen, r.d0.tolist())
        seen += c


def _rest(T, head):
    head = [int(c) for c in head]
    assert sum(head) < T, (T, head)
    return head + [T - sum(head)]


def _even(T, c):
    n = (T - 1) // c
    return [c] * n + [T - c * n]


def _random_split(rng, T, N):
    out = []
    while sum(out) < T:
        out.append(min(int(rng.integers(1, 2 * N + 1)), T - sum(out)))
    return out


def _row_len(kind, nb, T, N):
    return 64 * (_lib.lib().ofs_win_plan(KIND[kind], _lib.C64, _lib.FP32, nb, T, N) // 10)


def _chunkings(kind, W, nb, T, N):
    """The whole stream; one row per push; RL - 1 and RL + 1; cuts exactly at N - 2, N - 1 and N; five
    seeded random splits with pieces from 1 to 2N; for W = 128 the first 2N + 5 samples one at a time."""
    RL = _row_len(kind, nb, T, N)
    rng = np.random.default_rng(1000 * W + KIND[kind] + 10 * nb)
    out = [[T], _even(T, RL), _even(T, RL - 1), _even(T, RL + 1), _rest(T, [N - 2, 1, 1])]
    out += [_random_split(rng, T, N) for _ in range(5)]
    if W == 128:
        out.append(_rest(T, [1] * (2 * N + 5)))
    return out


def _detector(kind, B, nb, N, **kw):
    return _metrics.WindowMetricChunked(kind, B, nb, N, **kw)


# ------------------------------------------------------------------------------------------
# 1. any chunking equals the one-shot call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 256, 512, 1024, 2048])
@pytest.mark.parametrize("kind", ["sc", "comb", "minn"])
def test_any_chunking_equals_one_shot(kind, W):
    """W = 128 (E 2, MW 1), 256 (E 4, MW 1), 512 (MW 2), 1024 (MW 4), 2048 (MW 8); B = 5 streams (more than
    the 4 of one workgroup; 3 for Minn at W = 2048), T = 3N + 37 (odd); the same object throughout: each
    final call leaves fresh streams for the next chunking."""
    N = _N(kind, W)
    B, T = (3 if (kind == "minn" and W == 2048) else 5), 3 * _N(kind, W) + 37
    plan = _lib.lib().ofs_win_plan(KIND[kind], _lib.C64, _lib.FP32, 1, T, N)
    assert plan == {128: 21, 256: 41, 512: 42, 1024: 44, 2048: 48}[W], plan
    ref = _ref(kind, W, 1, B, T)
    xt = _stream(W, 1, B, T)
    det = _detector(kind, B, 1, N)
    runs = []
    for i, chunks in enumerate(_chunkings(kind, W, 1, T, N)):
        assert sum(chunks) == T and min(chunks) >= 1
        runs.append((chunks, _feed(det, _cut(xt, chunks), final=True, flush=(i % 2 == 1))))
        assert det.samples_seen == 0
    torch.cuda.synchronize()
    for chunks, res in runs:
        _assert_equal(res, ref, N, what=f"{kind} W={W} chunks {chunks[:6]}... ({len(chunks)})")
        _assert_d0(res, chunks, N, what=f"{kind} W={W} chunks {chunks[:6]}...")


# ------------------------------------------------------------------------------------------
# 2. two branches
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 512, 1024])
@pytest.mark.parametrize("kind", ["sc", "comb", "minn"])
def test_two_branches(kind, W):
    N = _N(kind, W)
    B, T = 5, 3 * N + 37
    ref = _ref(kind, W, 2, B, T)
    xt = _stream(W, 2, B, T)
    det = _detector(kind, B, 2, N)
    rng = np.random.default_rng(W + KIND[kind])
    splits = [_random_split(rng, T, N) for _ in range(5)] + [_rest(T, [N - 1, 1])]
    runs = [(c, _feed(det, _cut(xt, c))) for c in splits]
    torch.cuda.synchronize()
    for chunks, res in runs:
        _assert_equal(res, ref, N, what=f"2 branches {kind} W={W} chunks {chunks[:6]}...")
        _assert_d0(res, chunks, N)


# ------------------------------------------------------------------------------------------
# 3. outputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sc", "comb", "minn"])
def test_requested_outputs(kind):
    """Any subset of M / P / R is bitwise that of the full call; with outputs=() nothing is stored and
    the state still advances: a storing object that takes the state over continues the stream."""
    W, B = 256, 6
    N = _N(kind, W)
    T = 3 * N + 37
    ref = _ref(kind, W, 1, B, T)
    xt = _stream(W, 1, B, T)
    chunks = _rest(T, [N + 11, 1, 300, 255])
    pieces = _cut(xt, chunks)
    runs = []
    for want in (("M",), ("P", "R")):
        res = _feed(_detector(kind, B, 1, N, outputs=want), pieces)
        assert all(getattr(r, k) is None for r in res for k in KEYS if k not in want)
        runs.append((want, res))
    none = _detector(kind, B, 1, N, outputs=())
    quiet = _feed(none, pieces[:3], final=False)
    assert all(r.M is None and r.P is None and r.R is None for r in quiet) and none.samples_seen == sum(chunks[:3])
    full = _detector(kind, B, 1, N)
    full.state.copy_(none.state)
    tail = _feed(full, pieces[3:])
    torch.cuda.synchronize()
    for want, res in runs:
        _assert_equal(res, ref, N, keys=want, what=f"outputs {want}")
    _assert_d0(quiet, chunks[:3], N, what="outputs ()")
    s = sum(chunks[:3])
    assert tail[0].d0.tolist() == [s - (N - 1)] * B
    for k in KEYS:
        got = torch.cat([getattr(r, k) for r in tail], dim=1)
        assert torch.equal(_bits(got), _bits(ref[k][:, s - (N - 1):])), k


# ------------------------------------------------------------------------------------------
# 4. fill phase and d0
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sc", "comb", "minn"])
def test_fill_phase_is_zero_for_any_input(kind):
    """d < 0: all-zero bits also when the first samples are NaN or Inf, whatever the chunking; d0 =
    n_seen - (N - 1) on every call.  The stream without such samples equals its one-shot call."""
    W, B = 128, 5
    N = _N(kind, W)
    T = 2 * N + 131
    x = _stream(W, 1, B, T).clone()
    x[0, 0, 0] = float("nan")
    x[1, 0, 5] = complex(float("inf"), 0.0)
    x[2, 0, N - 2] = complex(0.0, float("nan"))
    x[3, 0, W] = complex(float("-inf"), 1.0)
    ref = _one_shot(kind, x, N)
    det = _detector(kind, B, 1, N)
    splits = ([T], _rest(T, [3] * (N // 3 + 2)), _rest(T, [N - 2, 1, 1, 1]), _rest(T, [1, W - 1, W + 1]))
    runs = [(c, _feed(det, _cut(x, c), flush=True)) for c in splits]
    torch.cuda.synchronize()
    for chunks, res in runs:
        _assert_d0(res, chunks, N, what=f"fill {chunks[:5]}")
        for k in KEYS:
            head = torch.cat([getattr(r, k) for r in res[:-1]], dim=1)[:, :N - 1]
            assert head.shape[1] == N - 1 and not bool(_bits(head).any()), (k, chunks[:5])
        _assert_equal(res, ref, N, rows=(4,), what=f"fill {chunks[:5]}")


# ------------------------------------------------------------------------------------------
# 5. partial reset: streams at different n in one launch
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,W", [("sc", 128), ("comb", 512), ("minn", 256)])
def test_partial_reset(kind, W):
    """reset(mask) / a memset of state rows after two chunks: the reset streams continue as a one-shot
    call on the remaining samples (indices from 0, rows aligned to the new start, their own fill
    phase), the others are unaffected."""
    B = 6
    N = _N(kind, W)
    T = 4 * N + 91
    s = N + 2 * W // 3 + 5                                             # not a row boundary
    chunks = [s - 77, 77] + _rest(T - s, [N - 3, 5, W + 1])
    ref = _ref(kind, W, 1, B, T)
    x = _stream(W, 1, B, T)
    tail = _one_shot(kind, x[:, :, s:].contiguous(), N)
    pieces = _cut(x, chunks)
    det = _detector(kind, B, 1, N)
    res = _feed(det, pieces[:2], final=False)
    det.reset(torch.tensor([True, False, False, True, False, False]))
    det.state[4].zero_()                                               # the documented memset of a state row
    res += _feed(det, pieces[2:], final=True)
    torch.cuda.synchronize()
    _assert_equal(res, ref, N, rows=(1, 2, 5), what="kept")
    _assert_equal(res[2:], tail, N, rows=(0, 3, 4), what="reset")
    assert res[2].d0.tolist() == [-(N - 1) if b in (0, 3, 4) else s - (N - 1) for b in range(B)]
    assert res[3].d0.tolist() == [chunks[2] - (N - 1) + (0 if b in (0, 3, 4) else s) for b in range(B)]
    det.push(pieces[0])
    det.reset()
    assert det.samples_seen == 0 and not bool(det.state.any())


# ------------------------------------------------------------------------------------------
# 6. final and flush
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sc", "comb", "minn"])
def test_final_and_flush_leave_fresh_streams(kind):
    """A stream abandoned in the middle by push(final=True) or flush(): the next push starts a fresh
    stream; final changes no output of its own call."""
    W, B = 512, 5
    N = _N(kind, W)
    T = 3 * N + 37
    ref = _ref(kind, W, 1, B, T)
    xt = _stream(W, 1, B, T)
    cut = N + 2 * W + 17
    head = _one_shot(kind, xt[:, :, :cut].contiguous(), N)
    det = _detector(kind, B, 1, N)
    pieces = _cut(xt, _rest(T, [700, cut - 700]))
    a = _feed(det, pieces[:2], final=True)                             # ends after `cut` samples
    assert det.samples_seen == 0
    b = _feed(det, _cut(xt, _rest(T, [N, 333])), final=False)           # a fresh stream: the whole input
    assert det.samples_seen == T
    f = _snap(det.flush())
    c = _feed(det, pieces, final=False)
    det.flush()
    d = _feed(det, [xt], final=True)
    torch.cuda.synchronize()
    _assert_equal(a, head, N, what="ended by final")
    _assert_equal(b, ref, N, what="after final")
    assert f.d0.tolist() == [T - (N - 1)] * B
    _assert_equal(c, ref, N, what="after flush")
    _assert_equal(d, ref, N, what="after flush, one push")


# ------------------------------------------------------------------------------------------
# 7. non-finite samples
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sc", "comb", "minn"])
def test_non_finite_samples(kind):
    """One NaN and, in another stream, one +Inf sample at n = N + 3: bitwise equal where the one-shot
    word is not NaN, the same NaN payload where it is (the sign of a NaN is outside the guarantee: it
    depends on the operand order of an add of two NaNs, which is the compiler's)."""
    W, B = 256, 5
    N = _N(kind, W)
    T = 3 * N + 37
    x = _stream(W, 1, B, T).clone()
    x[1, 0, N + 3] = float("nan")
    x[2, 0, N + 3] = complex(float("inf"), 0.0)
    ref = _one_shot(kind, x, N)
    for b in (1, 2):                                           # (Minn's M clips a NaN away: fmaxf)
        assert bool(torch.isnan(torch.view_as_real(ref["P"][b])).any()) and bool(torch.isnan(ref["R"][b]).any()), b
    assert bool(torch.isfinite(ref["M"][0]).all()) and bool(torch.isfinite(ref["R"][0]).all())
    det = _detector(kind, B, 1, N)
    rng = np.random.default_rng(5)
    splits = [[T], _rest(T, [N + 3, 1]), _rest(T, [N + 4, 255, 257]), _random_split(rng, T, N), _even(T, 255)]
    runs = [(c, _feed(det, _cut(x, c))) for c in splits]
    torch.cuda.synchronize()
    for chunks, res in runs:
        _assert_equal(res, ref, N, what=f"non-finite {chunks[:5]}", nan_sign_free=True)
        _assert_equal(res, ref, N, rows=(0, 3, 4), what=f"finite streams {chunks[:5]}")


# ------------------------------------------------------------------------------------------
# 8. against the fp64 oracle
# ------------------------------------------------------------------------------------------
def _check_model(kind, xh, N, M, P, R, Mo, Po, Ro, north_star):
    """Every output within error model 1 (tests/error_models.py), as tests/test_gpu_winfast.py checks
    the one-shot call; returns max |error| / bound over M, P, R."""
    bM, bP, bR = EM.window_model(kind, xh, N, Po, Ro, Mo)
    rM = np.abs(M.astype(np.float64) - Mo) / bM
    rP = np.abs(P.astype(np.complex128) - Po) / bP
    rR = np.abs(R.astype(np.float64) - Ro) / bR
    worst = float(max(rM.max(initial=0), rP.max(initial=0), rR.max(initial=0)))
    assert worst <= 1.0, (kind, float(rM.max()), float(rP.max()), float(rR.max()))
    if north_star:
        assert bool(np.all(np.abs(M - Mo) <= 1e-6 * np.maximum(1.0, np.abs(Mo))))
    return worst


@pytest.mark.parametrize("kind", ["sc", "comb", "minn"])
def test_against_fp64_oracle(kind):
    """The chunked outputs of one random split lie within the fp32 error model of the one-shot fast
    path (the same bound, no extra margin: the values are the same bits)."""
    W, B = 512, 6
    N = _N(kind, W)
    T = 3 * N + 37
    xt = _stream(W, 1, B, T)
    det = _detector(kind, B, 1, N)
    chunks = _random_split(np.random.default_rng(8), T, N)
    res = _feed(det, _cut(xt, chunks))
    torch.cuda.synchronize()
    got = {k: torch.cat([getattr(r, k) for r in res], dim=1)[:, N - 1:].cpu().numpy() for k in KEYS}
    xh = xt.cpu().numpy().astype(np.complex128)
    worst = 0.0
    for b in range(B):
        Mo, Po, Ro = ORACLE[kind](xh[b], N)
        worst = max(worst, _check_model(kind, xh[b], N, got["M"][b], got["P"][b], got["R"][b], Mo, Po, Ro,
                                        north_star=b != B - 1))          # the last stream holds the 60 dB step
    print(f"{kind} N={N} T={T} chunks {chunks}: max |err|/bound = {worst:.3g}")


# ------------------------------------------------------------------------------------------
# 9. back to back
# ------------------------------------------------------------------------------------------
def test_chunks_enqueued_without_host_synchronisation():
    """16 pushes of two objects of different kind, interleaved on one stream ([B, Tc] input for one
    branch, uploaded beforehand, each result cloned on the same stream), one synchronisation at the end."""
    W, B = 256, 5
    N1, N3 = _N("sc", W), _N("minn", W)
    T = 3 * N3 + 37
    ref1, ref3 = _ref("sc", W, 1, B, T), _ref("minn", W, 1, B, T)
    xt = _stream(W, 1, B, T)
    chunks = _rest(T, [197] * 15)
    pieces = [p[:, 0].contiguous() for p in _cut(xt, chunks)]
    d1, d3 = sc.SCChunkedMetric(B, 1, N1), minn.MinnChunkedMetric(B, 1, N3)
    torch.cuda.synchronize()
    r1, r3 = [], []
    for i, p in enumerate(pieces):                             # nothing below waits for the GPU
        r1.append(_snap(d1.push(p, final=i == 15)))
        r3.append(_snap(d3.push(p, final=i == 15)))
    torch.cuda.synchronize()
    assert len(pieces) == 16
    _assert_equal(r1, ref1, N1, what="back to back sc")
    _assert_equal(r3, ref3, N3, what="back to back minn")


def test_sc_minn_pair_equals_the_two_one_shot_calls():
    """combined_sc_min.SCMinnChunkedMetrics: both metrics from the same chunks (two launches per push),
    each equal to its own one-shot call."""
    W, B = 512, 5                                              # N = 2048: Minn window 512, S&C window 1024
    N = 4 * W
    T = 3 * N + 37
    xt = _stream(W, 1, B, T)
    ref_m, ref_s = _ref("minn", W, 1, B, T), _one_shot("comb", xt, N)
    both = combined_sc_min.SCMinnChunkedMetrics(B, 1, N)
    chunks = _random_split(np.random.default_rng(3), T, N)
    rm, rs = [], []
    for i, p in enumerate(_cut(xt, chunks)):
        m, s = both.push(p, final=i == len(chunks) - 1)
        rm.append(_snap(m))
        rs.append(_snap(s))
    torch.cuda.synchronize()
    _assert_equal(rm, ref_m, N, what="pair minn")
    _assert_equal(rs, ref_s, N, what="pair sc")
