"""CPU: the exact CP-search streams of tests/cp_streams.py are what they claim to be.

check() passes: every sample is a small integer that int16 and float32 hold, the oracle's P equals the exact
integer window sum bit for bit (in robust mode the sum over the range), the windows that share the largest
|P|^2 of a range are bit-identical or axis-aligned and every |P|^2 is below 2^44, the kernel's three-stage
decision restated without a mutation equals the oracle on every stream, and every tie, range size, clip,
empty range and non-finite pattern a configuration can hold (cp_streams.required) is present in the oracle's
output.  Every mutant - one wrong decision each - changes the expected result of at least one stream of the
family built for it, so a kernel making that error cannot pass tests/test_gpu_cp_exact.py.
"""
import math

import numpy as np

import cp_streams as S
import ofdm_oracle as O


def test_preconditions_and_coverage():
    got = S.check()
    cs = S.cases()
    for fam in sorted({c.family for c in cs}):
        sel = [c for c in cs if c.family == fam]
        print(f"family {fam}: {sum(len(c.names) for c in sel)} streams in {len(sel)} launches")
    for cfg, fs in got.items():
        print(f"facts {cfg}: {len(fs)}, streams per fact {dict(sorted(fs.items()))}")
    assert set(got) == set(S.CONFIGS) | {"cfo"}
    sizes = {len(c.names) for c in cs}
    assert 1 in sizes and 211 in sizes and max(sizes) <= 400, sizes


def test_every_mutant_is_caught():
    caught = S.mutants_caught()
    assert {k[0] for k in caught} == set(S.MUTANTS) and len(S.MUTANTS) == 12
    assert {(m, *v) for m, v in S.MUTANTS.items()} | set(S.TARGETS) == set(caught)
    for (mut, mode, fam), hit in caught.items():
        print(f"{mut} in mode {mode} by family {fam}: {len(hit)} streams, e.g. {hit[:2]}")
        assert hit, (mut, mode, fam)
    # the tie mutants are caught in every configuration, not by one lucky shape
    for mut in ("ge", "larger_d_lanes", "larger_d_waves"):
        assert {h[:3] for h in caught[(mut, S.PEAK, "ties")]} == set(S.CONFIGS), mut


def test_stated_examples():
    """What the kernels are held to on non-finite and empty ranges, as the oracle (pinned to the reference by
    tests/golden/cp_search_exact.npz) states it."""
    nan = S.NAN
    x = np.arange(1.0, 61.0) + 0j
    # N = 16, cp_len = 8, default span 4: the range [16, 24) is cp_len wide and sample 23 lies in every window
    y = x.copy()
    y[23] = nan
    cfo, d = O.cp_cfo_peak(y, 20, 16, 8, 1e6)
    assert d == 16 and cfo == 0 and math.copysign(1.0, cfo) < 0
    assert O.find_cp_start(y, 20, 16, 8, 4) == 16
    assert O.cp_search(y, 20, 16, 8, 4, 1, 1e6)[:3] == (0, 16, 0j)
    assert O.cp_search(np.full(60, nan + 0j), 20, 16, 8, 4, 1, 1e6)[:3] == (0, 16, 0j)
    y = x.copy()
    y[16] = nan                                             # only the window at 16 holds it: skipped
    assert O.cp_cfo_peak(y, 20, 16, 8, 1e6)[1] == 23 and O.cp_cfo_peak(x, 20, 16, 8, 1e6)[1] == 23
    st, d, P, cfo = O.cp_search(x, 20, 16, 8, 0, 1, 1e6)    # span 0: empty
    assert (st, d) == (1, 20) and math.isnan(P.real) and math.isnan(P.imag) and math.isnan(cfo)
    assert O.cp_search(x[:23], 0, 16, 8, 4, 0, 1e6)[0] == 1  # T < N + w
    assert O.cp_search(np.zeros(60, complex), 20, 16, 8, 4, 0, 1e6)[1:3] == (20, 0j)


def test_streams_are_shared_and_read_only():
    a = S.cases()
    assert a is S.cases() and not a[0].x.flags.writeable and not a[0].est.flags.writeable
    assert S.expected(0) is S.expected(0)
