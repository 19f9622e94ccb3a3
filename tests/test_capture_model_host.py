"""CPU: the plain-Python model of the frame capture (tests/capture_model.py) against slices of the whole
stream, and the scenarios the GPU test uses: no GPU case passes vacuously."""
import numpy as np
import pytest

import capture_model as cm


@pytest.mark.parametrize("F,H", cm.SIZES)
def test_clean_triggers_give_slices_of_the_whole_stream_for_every_chunking(F, H):
    sc = cm.clean_scenario(F, H)
    assert sc.T >= 5 * H
    x = cm.make_stream("i16", 2, sc.T, seed=F * 1000 + H)
    want = {b: [val + sc.offset for bb, val, _ in sc.triggers if bb == b] for b in range(cm.B)}
    assert sum(len(v) for v in want.values()) == len(sc.triggers) == 10 and not want[3]
    chs = cm.chunkings(sc.T, F, H)
    assert {"primes", "Tc=H", "Tc>H", "one push"} <= set(chs) and (("one sample" in chs) == ((F, H) == (1, 1)))
    for name, chunks in chs.items():
        assert sum(chunks) == sc.T
        got = {b: [] for b in range(cm.B)}
        for out in cm.run_model(sc, chunks, x):
            for b, (starts, frames, dropped) in enumerate(out):
                assert dropped == [0, 0, 0], (name, b)
                for s, fr in zip(starts, frames):
                    assert np.array_equal(fr, x[b, :, s:s + F]), (name, b, s)
                    got[b].append(s)
        assert got == want, name                                  # every frame, in one order per stream


def test_clean_scenarios_cover_the_alignment_residues_and_the_ring_wrap():
    for F, H in cm.SIZES:
        sc = cm.clean_scenario(F, H)
        starts = [val + sc.offset for _, val, _ in sc.triggers]
        assert {s % 4 for s in starts} == {0, 1, 2, 3} and max(starts) > 4 * H
        d = {(b, val): dd for b, val, dd in sc.triggers}
        s1 = next(val for b, val, _ in sc.triggers if b == 1)
        assert d[(1, s1)] - (s1 + sc.offset) == H                 # the retention edge under one-sample pushes
    assert any(F % 4 and F % 2 for F, _ in cm.SIZES)              # F no multiple of either vector width


def test_each_edge_scenario_drops_exactly_what_the_rules_say():
    seen = np.zeros(3, dtype=int)
    names = set()
    for sc in cm.edge_scenarios():
        names.add(sc.name)
        assert sum(sc.chunks) == sc.T
        x = cm.make_stream("c64", 1, sc.T, seed=1)
        outs = cm.run_model(sc, sc.chunks, x)
        total = np.sum([d for out in outs for _, _, d in out], axis=0)
        assert tuple(total) == sc.expect_dropped, sc.name
        seen += total
        assert sum(len(s) for out in outs for s, _, _ in out) > 0, sc.name     # every scenario emits a frame
    assert (seen > 0).all()                                       # late, queue full, cut: each occurs
    assert {"ends_at_chunk_end", "retention_edge", "queue_full", "sixteen_in_one_call", "count_above_max",
            "final_cuts", "flush_cuts", "reset_mid_frame"} <= names


def _emissions(name):
    sc = next(s for s in cm.edge_scenarios() if s.name == name)
    outs = cm.run_model(sc, sc.chunks, cm.make_stream("c64", 1, sc.T))
    return [[(b, s) for b, (starts, _, _) in enumerate(out) for s in starts] for out in outs]


def test_edge_scenarios_emit_where_intended():
    assert _emissions("ends_at_chunk_end") == [[], [(0, 13)], [(1, 14)], []]          # s + F == n1, and one later
    assert _emissions("retention_edge") == [[], [(0, 18)]]
    assert _emissions("offset_below_zero") == [[(3, 0)], []]
    assert _emissions("queue_full") == [[], [(0, 20), (0, 22)]]
    assert _emissions("queue_stays_full") == [[], [], [], [(1, 28), (1, 29)]]
    assert [len(e) for e in _emissions("sixteen_in_one_call")] == [0, 0, 0, 0, 16]
    assert [len(e) for e in _emissions("staggered_completions")] == [0, 0, 4, 6, 6]
    assert _emissions("final_cuts") == [[], [(1, 33)]]
    assert _emissions("flush_cuts")[-1] == []
    # streams 1 and 3 were reset before push 2: 0 and 2 complete there, 3 gets a frame at its new index 2
    assert _emissions("reset_mid_frame") == [[], [], [(0, 18), (2, 17), (3, 2)], []]


def test_model_refuses_an_unretrievable_start():
    m = cm.CaptureModel(1, 1, 4, 4, 2)
    x = cm.make_stream("c64", 1, 40)[:1]
    m.push(x[:, :, :10])
    m.pend[0].append(2)                                           # behind the history: the rules never queue it
    with pytest.raises(AssertionError):
        m.push(x[:, :, 10:20])
