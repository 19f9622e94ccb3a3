"""CPU: the exact |corr| streams of tests/zc_gate_streams.py are what they claim to be.

For every (n, W) of tests/test_gpu_zc_exact_events.py and every hysteresis of its two lists, check() passes:
the oracle's state equals int64 arithmetic on c * 16, family M's flags are valid & (c >= 0.5), and every
edge of the gate machine that the shape can hold (zc_gate_streams.required: an arithmetic predicate per
fact) is present in the oracle's output.  Every mutant of the oracle changes flags, mask or events on at
least one stream at hysteresis 64 and 256, so a kernel making that error cannot pass the GPU comparison.
Oracle results are cached per (n, W, hysteresis) in zc_gate_streams.expected (functools.lru_cache).
"""
import numpy as np
import pytest

import zc_gate_streams as Z


@pytest.mark.parametrize("n,W", Z.SHAPES, ids=str)
def test_preconditions_and_coverage(n, W):
    for hyst in Z.hysts_fused(n) + Z.HYSTS_SEQ:
        got = Z.check(n, W, hyst)
        assert "silent" in got
    print(f"n={n} W={W}: {sum(len(b.names) for b in Z.streams(n, W, 64).values())} streams, "
          f"{len(Z.check(n, W, 64))} facts at hysteresis 64")


@pytest.mark.parametrize("hyst", [64, 256])
def test_every_mutant_is_caught(hyst):
    caught = Z.mutants_caught(1024, 128, hyst)
    assert set(caught) == set(Z.MUTANTS) and len(Z.MUTANTS) == 14
    for mut, pred in Z.MUTANTS.items():
        print(f"hysteresis {hyst} {mut}: {len(caught[mut])} streams, e.g. {caught[mut][:3]}")
        if pred(max(hyst, 1)):
            assert caught[mut], (hyst, mut)
        else:
            assert not caught[mut], (hyst, mut)             # the mutant equals the oracle at this Hp
    assert Z.MUTANTS["quiet_ignores_open_gate"](256) and caught["quiet_ignores_open_gate"]
    # only the mutant that cannot differ for Hp >= 127 is excused anywhere
    assert [m for m, p in Z.MUTANTS.items() if not p(256)] == ["one_close_per_chunk"]
    assert all(p(64) for p in Z.MUTANTS.values())


def test_stated_examples():
    """n = 1024, W = 128, a chain from 192: hysteresis 64 closes in lane 63 and reopens in lane 0 of the
    next chunk; a constant 0.25 stream at thresh_value 256 is a tie at every valid sample, flagged above."""
    bt = Z.streams(1024, 128, 64)["M"]
    e = Z.expected(1024, 128, 64)["M"][bt.names.index("chain+64")]
    assert e["events"][0, :3].tolist() == [192, 192, 383] and e["events"][1, :2].tolist() == [384, 384]
    e = Z.run_oracle(Z._m(1024, [(192, 1.0), (255, 1.0), (319, 1.0), (384, 1.0)]), bt.params, 64)
    assert e["events"][:, :3].tolist() == [[192, 192, 383], [384, 384, 448]]
    e = Z.expected(1024, 128, 64)["M"][bt.names.index("min_chain")]
    assert len(e["events"]) > 8
    r = Z.run_oracle(np.full(1024, 0.25), (128, 256, 15, 0.0), 64)
    assert np.array_equal(r["corr_scaled"][128:], r["thresh_scaled"][128:]) and r["above_threshold"][128:].all()
    assert r["events"].tolist() == [[128, 128, 1024, 29]]


def test_streams_are_shared_and_read_only():
    a = Z.streams(1024, 128, 64)
    assert a is Z.streams(1024, 128, 64) and not a["M"].c.flags.writeable
    assert Z.expected(1024, 128, 64) is Z.expected(1024, 128, 64)
