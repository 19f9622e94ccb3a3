"""CPU: the NumPy model of the chunked zc_v2 CFAR + gate (tests/zc_chunk_model.py) against ofdm_oracle.

On the exact streams of tests/zc_gate_streams.py, for every split: the five state arrays, the events and
the peak values of the concatenated calls EQUAL the oracle's on the whole stream; every call's events
are the oracle's events whose gate_end falls among the call's samples (the end-of-stream close belongs
to the final call) and its open_gate_start is the start of the oracle gate that spans the call's end;
the concatenated gate_mask differs from the oracle's in no sample, or in exactly the one sample
open_gate_start < (start of the final call) - and both outcomes occur.
"""
import numpy as np
import pytest

import zc_chunk_model as M
import zc_gate_streams as Z

SHAPES = ((1024, 128), (1000, 128), (130, 128), (64, 32))


def hysts(n):
    return (0, 1, 63, 64, 65, 256, n + 7)


def model_splits(n, seed):
    def pieces(t):
        s = [t] * (n // t)
        return s + ([n - sum(s)] if n - sum(s) else [])
    out = [[n], [1, n - 2, 1], pieces(127), pieces(128), pieces(32)]
    rng = np.random.default_rng(seed)
    for _ in range(2):
        cuts = np.sort(rng.choice(np.arange(1, n), size=int(rng.integers(1, 8)), replace=False))
        out.append(np.diff(np.concatenate(([0], cuts, [n]))).astype(int).tolist())
    return out


def oracle_open_start(ev, t):
    """Start of the oracle gate that is open after sample t - 1 (its closing sample is >= t), or -1."""
    for pk, gs, ge, _ in ev.tolist():
        if gs < t <= ge:
            return gs
    return -1


def check_stream(c, params, hyst, e, split, tag, flush=False):
    """One stream, one split; returns True when the mask exception occurred."""
    n = len(c)
    calls = M.run_split(c, params, hyst, Z.REFLEN, split, flush=flush)
    got = M.concat(calls)
    for k in M.ARRAYS:
        assert np.array_equal(got[k], e[k]), (tag, k)
    assert np.array_equal(got["events"], e["events"]), (tag, got["events"].tolist(), e["events"].tolist())
    assert np.array_equal(got["peak_values"], e["peak_values"]), tag
    at = 0
    for j, d in enumerate(calls):
        t0, t1 = at, at + len(d["corr_mag"])
        last = j == len(calls) - 1
        ge = e["events"][:, 2]
        sel = (ge >= t0) & (ge < t1)
        if last:
            sel |= ge == n
        assert np.array_equal(d["events"], e["events"][sel]), (tag, j)
        assert d["n_events"] == int(sel.sum())
        assert d["open_gate_start"] == oracle_open_start(e["events"], t1), (tag, j, d["open_gate_start"])
        at = t1
    diff = np.flatnonzero(got["gate_mask"] != e["gate_mask"])
    exc = M.mask_exception(calls)
    if exc is None:
        assert diff.size == 0, (tag, diff[:8])
        return False
    assert diff.tolist() == [exc] and e["gate_mask"][exc] and not got["gate_mask"][exc], (tag, diff[:8], exc)
    return True


@pytest.mark.parametrize("n,W", SHAPES, ids=str)
def test_model_equals_oracle_under_every_split(n, W):
    seen = {True: 0, False: 0}
    for hyst in hysts(n):
        st, exp = Z.streams(n, W, hyst), Z.expected(n, W, hyst)
        for fam, bt in st.items():
            for k, split in enumerate(model_splits(n, 1000 * n + hyst)):
                for b, name in enumerate(bt.names):
                    hit = check_stream(bt.c[b], bt.params, hyst, exp[fam][b], split, (n, W, hyst, fam, name, k))
                    seen[hit] += 1
    assert seen[False] > 0
    if n > W + 2:
        assert seen[True] > 0, "no stream of this shape ends with a gate opened in an earlier call"


def test_flush_equals_final():
    """A Tc = 0 final call after the last chunk: the same events; the mask exception then covers every gate
    still open at the end (its start always lies before the empty call)."""
    n, W, hyst = 1000, 128, 256
    st, exp = Z.streams(n, W, hyst), Z.expected(n, W, hyst)
    hits = 0
    for fam, bt in st.items():
        for b, name in enumerate(bt.names):
            hits += check_stream(bt.c[b], bt.params, hyst, exp[fam][b], [333, 333, 334], (fam, name), flush=True)
    assert hits > 0


def test_state_is_fresh_after_final_and_carried_otherwise():
    n, W, hyst = 130, 128, 0
    bt = Z.streams(n, W, hyst)["M"]
    c = bt.c[bt.names.index("all_above")]
    m = M.ZCChunkModel(bt.params, hyst, Z.REFLEN)
    d = m.push(c[:129])
    assert m.n == 129 and m.open and d["open_gate_start"] == 128 and d["n_events"] == 0
    d = m.push(c[129:], final=True)
    assert d["n_events"] == 1 and d["events"][0].tolist() == [128, 128, 130, 29]
    acc, ring, cnt, gate, low = m.state_arrays()
    assert acc == 0.0 and not ring.any() and cnt == 0 and gate == (False, 0, 0, 0.0) and low == 0


def test_gpu_split_list_is_well_formed():
    for n, W in ((1024, 128), (2304, 1024), (130, 128), (64, 32), (1024, 100)):
        for s in M.splits(n, W, 7):
            assert sum(s) == n and min(s) >= 1
