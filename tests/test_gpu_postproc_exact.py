"""GPU: the detection post-processing kernels (csrc/postproc.hip) reproduce the oracle EXACTLY on the
exact metric streams of tests/post_streams.py.

Those streams hold multiples of 2^-4 and are smoothed over power-of-two windows, so every sum is exact in
any order and ties are real: equal maxima a lane, a wave and a whole stride apart, samples on exactly the
double 0.95 * max, 0.6 * peak, thr * max and M / max == thr, runs of exactly min_run and min_run - 1, two
longest runs of one length, run edges on, before and after the 256 per-thread chunk edges of
for_each_run, bounds that cut or remove a gate, and NaN, +inf and -inf in every position
(tests/test_post_streams_host.py proves the facts present and every single wrong decision caught).  One
rule, always against ofdm_oracle on the same stream (post_streams.expected): indices, gate bounds, spans,
masks and statuses are EQUAL and the smoothed metric is np.array_equal with NaNs equal by position (the sign
bit of a NaN is outside the guarantee).  Each case - a family at one length under one parameter set - is
one launch of the batched entry point, with float64 inputs and, where the kernel is templated, with the
same values as float32; the expected result of a float32 launch is the oracle on the float32 values.
"""
import numpy as np
import pytest
import torch

import post_streams as S
from ofdm_sync_amd import _postproc, combined_sc_min, minn, sc

pytestmark = pytest.mark.gpu

F32_OPS = ("plateau", "minn", "trail", "gate", "detect")     # segment_peak_kernel takes the f64 smoothed metric
OPS = ("plateau", "minn", "trail", "gate", "seg", "detect")


def launch(case, f32=False):
    """One call of the batched entry point of `case`; the result tuple of every stream, on the host."""
    dt = torch.float32 if f32 else torch.float64
    dev = lambda k: torch.from_numpy(np.array(case.data[k])).to("cuda", dt)   # noqa: E731  (a copy: read-only streams)
    h = lambda t: t.cpu().numpy()                                             # noqa: E731
    p, B = case.params, len(case.names)
    if case.op == "plateau":
        idx, Ms, st = (h(t) for t in sc.find_plateau_end_batched(dev("M"), p[0], lookahead=p[1], smooth_win=p[2]))
        return [(idx[b], st[b], Ms[b]) for b in range(B)]
    if case.op == "minn":
        pk, glo, ghi, Ms, st = (h(t) for t in minn.find_minn_peak_batched(dev("M"), p[0], p[1], p[2]))
        return [(pk[b], glo[b], ghi[b], st[b], Ms[b]) for b in range(B)]
    if case.op == "trail":
        y = h(_postproc.trailing_average(dev("x"), p[0], clip_negative=bool(p[1])))
        return [(y[b],) for b in range(B)]
    if case.op == "gate":
        mask, span = (h(t) for t in _postproc.sc_gate_batched(dev("M"), p[0]))
        return [(mask[b], span[b, 0], span[b, 1]) for b in range(B)]
    if case.op == "seg":
        mask = torch.from_numpy(np.array(case.data["mask"])).cuda()
        pk, st = (h(t) for t in _postproc.segment_peak_batched(dev("Ms"), mask, p[0]))
        return [(pk[b], st[b]) for b in range(B)]
    pk, st, span = (h(t) for t in combined_sc_min.detect_batched(dev("M_minn"), dev("M_sc"), smooth_win=p[0],
                                                                  threshold=p[1], search_bounds=p[2]))
    return [(pk[b], st[b], span[b, 0], span[b, 1]) for b in range(B)]


def brief(t):
    return tuple(x.tolist() if np.size(x) <= 8 else f"<{np.size(x)}>" for x in map(np.asarray, t))


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("n", S.NS)
def test_batched_entry_points_equal_the_oracle(n, op):
    """Every family, parameter set and stream of length n through the batched entry point of `op`."""
    ran = 0
    for f32 in (False, True) if op in F32_OPS else (False,):
        for case, exp in zip(S.cases(n), S.expected(n, f32)):
            if case.op != op:
                continue
            got = launch(case, f32)
            assert len(got) == len(exp) == len(case.names)
            for b, name in enumerate(case.names):
                assert S.same(got[b], exp[b]), (op, case.family, n, case.params, "f32" if f32 else "f64", name,
                                                brief(got[b]), brief(exp[b]))
            ran += len(got)
    print(f"n={n} {op}: {ran} streams")
    assert ran > 0


def test_drop_in_functions_equal_the_oracle():
    """The numpy-in drop-in functions on one stream of every case at n = 257 (a different stream from case
    to case), and on the first stream of every status the oracle raises for: the ValueErrors of status
    -1 (empty gate region), -2 (no positive peak) and -3 (numpy's broadcast error) included."""
    n = 257
    raised = set()
    picks = []
    for j, (case, exp) in enumerate(zip(S.cases(n), S.expected(n))):
        picks.append((case, exp, j % len(case.names)))
        for b in range(len(case.names)):
            st = {"plateau": 1, "minn": 3, "seg": 1, "detect": 1}.get(case.op)
            if st is not None and exp[b][st] < 0 and (case.op, exp[b][st]) not in raised:
                raised.add((case.op, exp[b][st]))
                picks.append((case, exp, b))
    assert raised == {("plateau", -3), ("minn", -2), ("seg", -1), ("detect", -1)}
    for case, exp, b in picks:
        p, e = case.params, exp[b]
        row = [np.array(a[b]) for a in case.data.values()]
        tag = (case.op, case.family, p, case.names[b])
        if case.op == "plateau":
            call = lambda: sc.find_plateau_end_from_metric(row[0], p[0], lookahead=p[1], smooth_win=p[2])  # noqa: E731
            if e[1] == -3:
                with pytest.raises(ValueError):
                    call()
            else:
                assert call() == e[0], tag
        elif case.op == "minn":
            call = lambda: minn.find_minn_peak(row[0], smooth_win=p[0], gate_threshold=p[1], search_bounds=p[2])  # noqa: E731
            if e[3] == -2:
                with pytest.raises(ValueError):
                    call()
            else:
                pk, gate, Ms = call()
                want = np.zeros(n, bool)
                want[e[1]:e[2]] = True
                assert pk == e[0] and np.array_equal(gate, want) and np.array_equal(Ms, e[4], equal_nan=True), tag
        elif case.op == "trail" and not p[1]:
            assert np.array_equal(minn._trailing_average(row[0], p[0]), e[0], equal_nan=True), tag
            assert np.array_equal(combined_sc_min._trailing_average(row[0], p[0]), e[0], equal_nan=True), tag
        elif case.op == "gate":
            mask, span = combined_sc_min.sc_gate_mask(row[0], p[0])
            assert np.array_equal(mask, e[0]) and span == (e[1], e[2]), tag
        elif case.op == "seg" and p[0] is None:
            r = combined_sc_min._streaming_peak_detector(row[0], row[1])
            assert (r is None and e[1] == -1) or (r == e[0] and e[1] == 0), tag
        elif case.op == "detect":
            mask, span = combined_sc_min.sc_gate_mask(row[1], p[1])
            assert span == (e[2], e[3]), tag
            call = lambda: combined_sc_min.find_minn_peak(row[0], smooth_win=p[0], gate_mask=mask, search_bounds=p[2])  # noqa: E731
            if e[1] == -1:
                with pytest.raises(ValueError):
                    call()
            else:
                assert call() == e[0], tag


def test_position_independence():
    """A stream's answers do not depend on its row: every plateau, minn and gate batch of n = 513 under one
    parameter set, reversed and cut to 1, 3 and 5 streams (the trailing average packs 4 per workgroup)."""
    n = 513
    done = set()
    for case, exp in zip(S.cases(n), S.expected(n)):
        if (case.op, case.family) in done or case.op == "seg":
            continue
        done.add((case.op, case.family))
        B = len(case.names)
        for order in (list(range(B))[::-1], [B - 1], [2, 0, 1], [4, 3, 2, 1, 0]):
            sub = S.Case(case.op, case.family, n, case.params, [case.names[b] for b in order],
                         {k: a[np.array(order)] for k, a in case.data.items()})
            got = launch(sub)
            for j, b in enumerate(order):
                assert S.same(got[j], exp[b]), (case.op, case.family, case.params, case.names[b], order[:5])
