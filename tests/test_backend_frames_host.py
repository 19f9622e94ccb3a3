"""Host checks of tests/backend_frames.py (no GPU): the model is the oracle on interior frames, its stream-edge
rule agrees with itself, and on every shape of test_gpu_backend_exact.py it stays inside the tolerances of the
closed forms - the evidence that the GPU test's reference cannot itself use up a tolerance."""
import functools

import numpy as np
import pytest

import backend_frames as F
import ofdm_oracle as O


def bits(v):
    return np.ascontiguousarray(np.asarray(v, np.complex128 if np.iscomplexobj(v) else np.float64)).view(np.uint64)


@pytest.mark.parametrize("nb,N", [(1, 2048), (2, 1024), (3, 256), (2, 4096), (2, 2048)])
def test_model_is_the_oracle_on_interior_frames(nb, N):
    """The random integer frames of test_gpu_parity.py::test_receiver_backend_batched_vs_oracle, estimated and
    given CFO: every output array for array (value equality: a -0.0 equals 0.0)."""
    rng = np.random.default_rng(N + nb)
    B, cp = 6, N // 4
    k = F.centered(N // 2)
    T = 2 * (N + cp) + 400
    x = np.round((rng.standard_normal((B, nb, T)) + 1j * rng.standard_normal((B, nb, T))) * 300)
    ps = rng.integers(0, 100, B)
    ds = ps + N + cp
    pil = np.exp(2j * np.pi * rng.random((B, k.size)))
    dat = np.exp(2j * np.pi * rng.random(k.size))
    for b in range(B):
        for cfo in (None, 1234.5):
            r = O.rx_backend(x[b], int(ps[b]), int(ds[b]), N, cp, 1e6, k, pil[b], dat, cfo=cfo)
            m = F.model(x[b], int(ps[b]), int(ds[b]), N, cp, 1e6, k, pil[b], dat, cfo=cfo)
            for key in F.KEYS:
                np.testing.assert_array_equal(np.asarray(m[key]), np.asarray(r[key]), err_msg=key)


@pytest.mark.parametrize("shape", F.EDGE_SHAPES, ids=str)
@pytest.mark.parametrize("short", [False, True], ids=["long", "short"])
def test_edge_rule_agrees_with_itself(shape, short):
    """A cut frame equals the same frame inside the zero-padded stream at origin -P: bit for bit with the CFO
    given, and with the CFO estimated apart from the sign of a zero cfo.  The wholly-outside frame is pinned."""
    N, U, cp, nb, name = shape
    k = F.bin_sets(N, U)[name]
    x, ps, ds, what, pil, dat, cfo = F.edge_batch(N, U, cp, nb, short)
    P = F.edge_pad(N, cp)
    for b in range(x.shape[0]):
        for c in (None, float(cfo[b])):
            a = F.model(x[b], int(ps[b]), int(ds[b]), N, cp, F.FS, k, pil[b], dat, cfo=c)
            p = F.model(F.pad(x[b], P), int(ps[b]) + P, int(ds[b]) + P, N, cp, F.FS, k, pil[b], dat, cfo=c, origin=-P)
            for key in F.KEYS:
                if key == "cfo" and c is None and a["cfo"] == 0.0 and p["cfo"] == 0.0:
                    continue
                assert np.array_equal(bits(a[key]), bits(p[key])), (key, b, what[b], c)
            assert all(np.all(np.isfinite(np.asarray(a[key]))) for key in F.KEYS), (b, what[b])
        if ps[b] + cp + N <= 0 and ds[b] + cp >= x.shape[2] and not short:
            a = F.model(x[b], int(ps[b]), int(ds[b]), N, cp, F.FS, k, pil[b], dat)
            assert bits(a["cfo"]) == bits(-0.0) and not np.any(a["h"]) and a["gain"] == 0 and a["evm"] == 1.0
            assert not np.any(a["xa"]) and abs(a["evm_db"]) < 1e-11
            assert set(np.abs(np.angle(a["h"]))) <= {0.0, np.pi}


def test_edge_positions_cut_what_they_say():
    """The positions reach every arm: CP pairs partly, singly and wholly dropped, either window cut at either
    end and wholly outside, a thread's stride inside the window."""
    N, cp = 1024, 72
    T = 2 * (N + cp) + 8
    pos = F.edge_positions(N, cp, T)
    pairs = [int(np.sum((p + np.arange(cp) >= 0) & (p + N + np.arange(cp) < T))) for p, _, _ in pos]
    assert {0, 1, cp - 1, cp} <= set(pairs)
    inside = lambda s: int(np.sum((s + cp + np.arange(N) >= 0) & (s + cp + np.arange(N) < T)))
    pw, dw = [inside(p) for p, _, _ in pos], [inside(d) for _, d, _ in pos]
    assert {0, 1, N - 1, N} <= set(pw) and {0, 1, N - 1, N - cp, N} <= set(dw)
    assert any(p == 0 and d == 0 for p, d in zip(pw, dw))
    assert len(pos) <= 256 and all(len(F.edge_positions(s[0], s[2], 2 * (s[0] + s[2]) + 8)) <= 256 for s in F.EDGE_SHAPES)
    assert {-(cp + N + 3), 3} <= {p for p, _, w in pos if w == "head"}
    assert {p for p, _, w in F.edge_positions(64, 16, 168) if w == "head"} == set(range(-(16 + 64 + 3), 4))


@functools.lru_cache(maxsize=None)
def delay_results(shape):
    """[(bin set, model outputs, closed forms)] of one delay shape, each stacked over its delays."""
    N, U, cp, branches, count = shape
    out = []
    for name, k in F.bin_sets(N, U).items():
        d = F.odd_delays(N, k, count)
        assert d.size <= 256
        x, ps, ds = F.delay_batch(N, cp, branches[-1], d)
        r = F.stack([F.model(x[b], int(ps[b]), int(ds[b]), N, cp, F.FS, k, np.ones(U), F.data_ref(U), cfo=0.0)
                     for b in range(d.size)])
        out.append((name, r, F.stack([F.delay_closed_form(N, k, di) for di in d])))
    return out


@pytest.mark.parametrize("shape", F.DELAY_SHAPES, ids=str)
def test_delay_frames_meet_their_closed_forms(shape):
    """The model on every delay frame of the GPU test against the closed forms, at the GPU test's tolerances.  A
    single bin (U = 1) always aligns exactly: its evm is the 1e-12 of the gain's denominator where the closed
    form says 0, so the closed form's evm_db (-240 against the oracle's -233.98) is left out there."""
    N, U = shape[:2]
    for name, r, c in delay_results(shape):
        dev, tol = F.batch_deviations(r, c), F.batch_tolerances(c, N)
        for key in F.KEYS:
            if not (U == 1 and key == "evm_db"):
                assert np.all(dev[key] < tol[key]), (name, key, float(dev[key].max()))
        assert np.all(r["cfo"] == 0.0)
        if U == 1:
            assert np.all(r["slope"] == 0.0) and np.all(r["evm"] < 1.1e-12)


def test_the_reference_error_is_far_inside_the_tolerances():
    """Worst over every delay shape and bin set with U >= 2 (measured: see the assertion's message):
    |sto - d| 1.8e-11, |evm - closed form| 7.1e-13, |gain - mean(ref)| 8.0e-10 - the last is the 1e-9 of
    h + 1e-9 (xhat = 1 + 1e-9), not rounding.  The tolerances are sto 1.6e-7·N/1024 at least, evm 1e-8,
    gain 1e-8."""
    sto = evm = gain = 0.0
    for shape in F.DELAY_SHAPES:
        if shape[1] >= 2:
            for _, r, c in delay_results(shape):
                dev = F.batch_deviations(r, c)
                sto, evm, gain = max(sto, dev["sto"].max()), max(evm, dev["evm"].max()), max(gain, dev["gain"].max())
    print(f"worst |sto - d| {sto:.3g}, |evm - closed| {evm:.3g}, |gain - mean(ref)| {gain:.3g}")
    assert sto < 1e-10 and evm < 1e-11 and gain < 1.1e-9, (sto, evm, gain)


@pytest.mark.parametrize("shape", F.TIE_SHAPES, ids=str)
def test_tie_frames_have_their_properties(shape):
    """h exactly real, phases in {-pi, 0}, np.unwrap returns them unchanged; dropping the boundary rule would
    move the slope by far more than its tolerance."""
    N, U, cp, nb = shape
    pil = F.tie_pilots(U)
    x, ps, ds = F.delay_batch(N, cp, nb, [0, 0, 0])
    for name, k in F.bin_sets(N, U).items():
        for b in range(3):
            r = F.model(x[b], int(ps[b]), int(ds[b]), N, cp, F.FS, k, pil[b], F.data_ref(U), cfo=0.0)
            assert np.all(r["h"].imag == 0)
            assert np.array_equal(bits(r["h"]), bits((F.AMP + 0j) / (pil[b] + 1e-9)))
            ph = np.angle(r["h"])
            assert set(ph) <= {-np.pi, 0.0} and np.array_equal(np.unwrap(ph), ph)
            if b < 2:                                        # mixed signs: a +pi step exists, so the rule matters
                dd = np.diff(ph)
                lost = ph + np.concatenate(([0.0], np.cumsum(np.where(dd == np.pi, -2 * np.pi, 0.0))))
                kz = k - np.mean(k)
                wrong = float(np.sum(kz * (lost - np.mean(lost))) / (np.sum(kz * kz) + 1e-12))
                assert abs(wrong - r["slope"]) > 1e-2 * 2 * np.pi / N


def test_dispatch_pairs_are_in_both_tables():
    """cp_len 512 | 513, n_used 768 | 769, 2 | 3 branches: each side is a delay shape and an edge shape, the
    first on the fast kernel and the second on the generic one (nothing is compared across a pair)."""
    delay = {(N, U, cp, nb) for N, U, cp, branches, _ in F.DELAY_SHAPES for nb in branches}
    edge = {s[:4] for s in F.EDGE_SHAPES}
    for fast, generic in (((1024, 257, 512), (1024, 257, 513)), ((1024, 768, 72), (1024, 769, 72))):
        for table in (delay, edge):
            assert any(s[:3] == fast and F.is_fast(s[0], s[1], s[3], s[2]) for s in table)
            assert any(s[:3] == generic and not F.is_fast(s[0], s[1], s[3], s[2]) for s in table)
    for table in (delay, edge):
        assert (1024, 256, 72, 2) in table and (1024, 256, 72, 3) in table
    assert F.is_fast(1024, 256, 2, 72) and not F.is_fast(1024, 256, 3, 72)
