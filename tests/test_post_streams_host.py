"""CPU: the exact metric streams of tests/post_streams.py are what they claim to be.

For every length of tests/test_gpu_postproc_exact.py, check() passes: the values lie on the 2^-4 grid (the
level families hold, off the grid, nothing but the double 0.95 * max or 0.6 * peak, at w = 1), the oracle's
smoothed metric equals the kernel's ascending-order window sum bit for bit, the restated decision
functions without a mutation equal the oracle on every stream, and every tie, equality at a level,
plateau branch and run edge on a chunk boundary that the length can hold (post_streams.required: an
arithmetic predicate per fact) is present in the oracle's output.  Every mutant of the oracle - one wrong
decision each - changes the expected result of at least one stream of every entry point it touches, and
of the family built for that decision, so a kernel making that error cannot pass the GPU comparison.
Oracle results are cached per length in post_streams.expected (functools.lru_cache).
"""
import numpy as np
import pytest

import ofdm_oracle as O
import post_streams as S


@pytest.mark.parametrize("n", S.NS)
def test_preconditions_and_coverage(n):
    got = S.check(n)
    cs = S.cases(n)
    for fam in sorted({c.family for c in cs}):
        ops = sorted({c.op for c in cs if c.family == fam})
        streams = sum(len(c.names) for c in cs if c.family == fam)
        launches = sum(c.family == fam for c in cs)
        print(f"n={n} family {fam}: {streams} streams in {launches} launches ({', '.join(ops)})")
    for group, fs in got.items():
        print(f"n={n} facts {group}: {len(fs)} {sorted(fs)}")
    req = S.required(n)
    if n == 1025:                                            # nothing but the n < w fact is waived at the largest length
        assert [f for fs in req.values() for f, need in fs.items() if not need] == ["pl_n<w"]
    # the trailing average packs 4 streams per workgroup: some batches leave its last workgroup part empty
    sizes = {len(c.names) for c in cs}
    assert any(b % 4 for b in sizes) and max(sizes) <= 400, sizes


def test_every_mutant_is_caught():
    caught = S.mutants_caught()
    assert {k[0] for k in caught} == set(S.MUTANTS) and len(S.MUTANTS) == 22
    assert set(S.TARGETS) <= set(caught)
    for (mut, op, fam), hit in caught.items():
        print(f"{mut} in {op}{' by family ' + fam if fam else ''}: {len(hit)} streams, e.g. {hit[:2]}")
        assert hit, (mut, op, fam)
        if fam is None:                                      # finite decisions are caught by finite streams
            assert all((h[1] == "nonfinite") == (mut in S.NAN_MUTANTS) for h in hit), (mut, op)


def test_smoothed_metric_is_exact_in_any_order():
    """Dyadic random streams at every length, n < w included: np.convolve equals the ascending-order sum
    bit for bit, and so does the descending-order one."""
    rng = np.random.default_rng(77)
    count = 0
    for n in S.NS + (3, 15, 16, 17, 100):
        for w in S.WS:
            for _ in range(20):
                M = rng.integers(0, 17, n) / 16.0
                Ms = np.convolve(M, np.ones(w) / w, mode="same")
                assert Ms.size == max(n, w)
                assert np.array_equal(Ms, S.ms_ascending(M, w)), (n, w)
                assert np.array_equal(Ms, S.ms_ascending(M, w, descending=True)), (n, w)
                count += 1
    assert count >= 1200


def test_stated_examples():
    """The non-finite behaviour the kernels are held to, as the oracle (pinned to the reference by
    tests/golden/post_exact_*.npz) states it."""
    nan, inf = S.NAN, S.INF
    assert O.plateau_end(np.full(300, nan), 16, None, 8)[:2] == (2, 3)
    assert O.plateau_end(np.full(300, -inf), 16, None, 8)[:2] == (0, 1)
    assert O.sc_gate(np.full(300, nan))[1] == (0, 1) and O.sc_gate(np.full(300, -inf))[1] == (0, 1)
    assert O.sc_gate(np.array([0.5] * 100 + [nan] + [1.0] * 199))[1] == (101, 300)
    assert O.streaming_peak(np.array([1, nan, 3, 2.0]), [0, 1, 1, 1]) == 1
    assert O.streaming_peak(np.array([1, 2, nan, 3.0]), [0, 1, 1, 1]) == 3
    assert O.streaming_peak(np.full(4, -inf), [0, 1, 1, 0]) == 1
    pk, gate, _ = O.minn_peak(np.array([0.25, 0.5, nan, 1.0]), 1, 0.5)
    assert pk == 2 and gate.tolist() == [False, False, True, False]
    with pytest.raises(ValueError):
        O.minn_peak(np.full(8, -inf), 4, 0.5)
    # 3/5, 6/10 and 9/15 are exactly the double 0.6; the threshold one ulp above 1/3 separates / from *
    assert all(np.float64(v) / np.float64(m) == 0.6 for v, m in ((3, 5), (6, 10), (9, 15)))
    assert 1 / 16 / (3 / 16) < S.THR_MUL and 1 / 16 >= S.THR_MUL * (3 / 16)


def test_streams_are_shared_and_read_only():
    a = S.cases(257)
    assert a is S.cases(257) and not a[0].data["M"].flags.writeable
    assert S.expected(257) is S.expected(257)
    grid = [j for j, c in enumerate(a) if c.family == "metric"]
    assert all(S.expected(257, True)[j] is S.expected(257)[j] for j in grid)   # float32 holds the grid exactly
