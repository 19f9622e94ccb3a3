"""GPU: the zc_v2 CFAR + gate kernels reproduce the oracle EXACTLY on the exact |corr| streams of
tests/zc_gate_streams.py, in both output modes.

Every sample of those streams is a multiple of 2^-4, so the running sums, c * 2^f and local_sum * tv are
exact and ties in the CFAR comparison are real; the streams place gate edges on the first and last lane of
the fused kernel's 64-sample rows and 128-sample chunks, closes and reopens in one row, two closes in one
chunk, gaps of Hp - 1, Hp and Hp + 1, tails that close on or just beyond the last sample, peak ties and
peaks on non-above and closing samples (zc_gate_streams.check lists what a shape holds).  One rule for every
kernel form, always against ofdm_oracle on the same stream: gate_mask, n_events (also above max_events),
events[:k] and peak_values[:k] are EQUAL, with state arrays requested all five are EQUAL, and every event
slot at or beyond min(k, E) still holds the canary the buffers were filled with.  The call is the C ABI's
ofs_zc_detect with all streams of a family in one launch; each case first asserts which kernel serves it
(ofs_zc_detect_plan: 0 sequential, 1 register-staged tiles, 2 LDS-DMA events + mask only, 3 LDS-DMA with
state arrays).
"""
import numpy as np
import pytest
import torch

import zc_gate_streams as Z
from ofdm_sync_amd import _lib, zc_v2

pytestmark = pytest.mark.gpu

E = 16
CAN_I, CAN_F, CAN_U8, CAN_N = -77, -77.0, 0xA5, -5
STATE = (("local_sum", torch.float64), ("corr_scaled", torch.float64), ("thresh_scaled", torch.float64),
         ("above_threshold", torch.uint8), ("metric_valid", torch.uint8))


def plan(n, W, hyst, state, aligned=True):
    return int(_lib.lib().ofs_zc_detect_plan(n, W, hyst, int(state), int(aligned)))


def device_mag(c, misalign=False):
    """c [B][n] on the device, 16-byte aligned, or a contiguous view starting 8 bytes into its storage."""
    h = torch.from_numpy(np.array(c, np.float64))          # a copy: the shared streams are read-only
    if not misalign:
        d = h.cuda()
        assert d.data_ptr() % 16 == 0
        return d
    store = torch.empty(h.numel() + 1, dtype=torch.float64, device="cuda")
    d = store[1:].view(h.shape)
    d.copy_(h)
    assert d.is_contiguous() and d.data_ptr() % 16 == 8
    return d


def launch(mag, params, hyst, state, max_ev=E, reflen=Z.REFLEN):
    """One ofs_zc_detect call on canary-filled buffers; outputs as host arrays."""
    B, n = mag.shape
    W, tv, f, mn = params
    dev = mag.device
    out = {k: torch.full((B, n), CAN_F if dt == torch.float64 else CAN_U8, dtype=dt, device=dev)
           for k, dt in STATE} if state else {}
    gate = torch.full((B, n), CAN_U8, dtype=torch.uint8, device=dev)
    n_ev = torch.full((B,), CAN_N, dtype=torch.int32, device=dev)
    ev_i = torch.full((B, max_ev, 4), CAN_I, dtype=torch.int64, device=dev)
    ev_v = torch.full((B, max_ev), CAN_F, dtype=torch.float64, device=dev)
    p = lambda k: out[k].data_ptr() if k in out else None  # noqa: E731
    rc = _lib.lib().ofs_zc_detect(mag.data_ptr(), B, n, int(W), int(tv), int(f), float(mn), int(reflen), int(hyst),
                                  p("local_sum"), p("corr_scaled"), p("thresh_scaled"), p("above_threshold"),
                                  p("metric_valid"), gate.data_ptr(), max_ev, n_ev.data_ptr(), ev_i.data_ptr(),
                                  ev_v.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(gate_mask=gate.cpu().numpy(), n_events=n_ev.cpu().numpy(), events=ev_i.cpu().numpy(),
               peak_values=ev_v.cpu().numpy())
    return res


def compare(res, exp, names, state, tag, max_ev=E, order=None):
    """The one comparison rule (module docstring).  order[j]: the stream of `exp` in row j of the launch."""
    order = range(len(names)) if order is None else order
    assert len(res["n_events"]) == len(order)
    for j, b in enumerate(order):
        e, t = exp[b], (tag, names[b], j)
        assert np.array_equal(res["gate_mask"][j], e["gate_mask"].astype(np.uint8)), t
        assert res["n_events"][j] == len(e["events"]), (t, res["n_events"][j], len(e["events"]))
        k = min(len(e["events"]), max_ev)
        assert np.array_equal(res["events"][j, :k], e["events"][:k]), (t, res["events"][j, :k].tolist(),
                                                                       e["events"][:k].tolist())
        assert np.array_equal(res["peak_values"][j, :k], e["peak_values"][:k]), t
        assert np.all(res["events"][j, k:] == CAN_I) and np.all(res["peak_values"][j, k:] == CAN_F), t
        if state:
            for key in ("local_sum", "corr_scaled", "thresh_scaled"):
                assert np.array_equal(res[key][j], e[key]), (t, key)
            for key in ("above_threshold", "metric_valid"):
                assert np.array_equal(res[key][j], e[key].astype(np.uint8)), (t, key)


def run_case(n, W, hyst, want_plan, variants=None, misalign=False, max_ev=E, families=("M", "C")):
    """Both families x both output modes of one (shape, hysteresis, kernel form)."""
    st, exp = Z.streams(n, W, hyst), Z.expected(n, W, hyst)
    for fam in families:
        bt = st[fam]
        mag = device_mag(bt.c, misalign)
        for state in (True, False):
            with _lib.variants(**(variants or {})):
                got = plan(n, W, hyst, state, not misalign)
                assert got == (want_plan if want_plan != 2 or not state else 3), (n, W, hyst, state, got)
                res = launch(mag, bt.params, hyst, state, max_ev)
            compare(res, exp[fam], bt.names, state, (n, W, hyst, fam, "state" if state else "events only",
                                                      variants, misalign), max_ev)


@pytest.mark.parametrize("n,W", Z.SHAPES, ids=str)
def test_fused_kernel_both_modes(n, W):
    """Hysteresis 64, 65, 127, 128, 129, 256, 1000 and n + 7 on the fused kernel: LDS-DMA tiles (plan 3 with
    state arrays, plan 2 - the benchmarked events-only instantiation, whose helpers read c from the LDS
    tiles - without) where n and W are whole chunks, register-staged tiles (plan 1) elsewhere.  The
    LDS-DMA shapes also run with register-staged tiles (variant ZC_NODMA, and a corr_mag that starts
    8 bytes into its storage) and through the sequential kernel (variant ZC_SEQ)."""
    dma = (n, W) in Z.DMA_SHAPES
    for hyst in Z.hysts_fused(n):
        run_case(n, W, hyst, 2 if dma else 1)
        if dma:
            run_case(n, W, hyst, 1, variants={"ZC_NODMA": 1})
            run_case(n, W, hyst, 0, variants={"ZC_SEQ": 1})
            run_case(n, W, hyst, 1, misalign=True)


@pytest.mark.parametrize("n,W", Z.SHAPES, ids=str)
def test_sequential_kernel_both_modes(n, W):
    """Hysteresis 0, 1, 2 and 63: zc_detect_kernel (plan 0), with hundreds of events per stream at 0 and 1
    (the counts stay exact above max_events)."""
    for hyst in Z.HYSTS_SEQ:
        run_case(n, W, hyst, 0)


def test_plan_values():
    P = _lib.lib().ofs_zc_detect_plan
    assert P(1024, 128, 256, 0, 1) == 2 and P(1024, 128, 256, 1, 1) == 3
    assert P(1000, 128, 256, 0, 1) == 1 and P(1000, 128, 256, 1, 1) == 1
    assert P(1024, 128, 63, 0, 1) == 0 and P(1024, 128, 64, 0, 1) == 2
    assert P(1024, 128, 256, 0, 0) == 1 and P(1024, 100, 256, 0, 1) == 1
    with _lib.variants(ZC_NODMA=1):
        assert P(1024, 128, 256, 0, 1) == 1
    with _lib.variants(ZC_SEQ=1):
        assert P(1024, 128, 256, 0, 1) == 0
    assert P(1024, 128, 256, 0, 1) == 2


def test_event_overflow_keeps_count_and_canary():
    """(1024, 128, 64) with two event slots: n_events is the true count (> 8 on the minimal chain), the
    first two rows are right and the slots beyond hold the canary: LDS-DMA, register-staged, sequential."""
    n, W, hyst = 1024, 128, 64
    assert max(len(e["events"]) for e in Z.expected(n, W, hyst)["M"]) > 8
    run_case(n, W, hyst, 2, max_ev=2)
    run_case(n, W, hyst, 1, variants={"ZC_NODMA": 1}, max_ev=2)
    run_case(n, W, hyst, 0, variants={"ZC_SEQ": 1}, max_ev=2)
    run_case(1000, W, hyst, 1, max_ev=2)


@pytest.mark.parametrize("want_state", [True, False])
def test_regrowth_loop_returns_all_events(want_state):
    """detect_zc_preamble_batched(max_events=2) on the fused kernel: a one-tap reference and no
    normalisation make |corr| the family-M streams themselves; the regrowth loop returns every event."""
    n, W, hyst = 1024, 128, 64
    bt = Z.streams(n, W, hyst)["M"]
    x = torch.from_numpy(bt.c.astype(np.complex128)[:, None, :]).cuda()
    _, tv, f, mn = bt.params
    assert plan(n, W, hyst, want_state) == (3 if want_state else 2)
    r = zc_v2.detect_zc_preamble_batched(x, np.array([1.0 + 0j]), W, tv, f, mn, hyst, normalize=False,
                                         max_events=2, want_state=want_state)
    mag = r.corr_mag.cpu().numpy()
    assert mag.shape == bt.c.shape
    worst = int(r.n_events.max())
    assert worst > 8 and r.events.shape[1] == worst == r.peak_values.shape[1]
    for b, name in enumerate(bt.names):
        e = Z.run_oracle(mag[b], bt.params, hyst, reflen=1)
        k = int(r.n_events[b])
        assert k == len(e["events"]), name
        assert np.array_equal(r.events[b, :k].cpu().numpy(), e["events"]), name
        assert np.array_equal(r.peak_values[b, :k].cpu().numpy(), e["peak_values"]), name
        assert np.array_equal(r.gate_mask[b].cpu().numpy(), e["gate_mask"].astype(np.uint8)), name


@pytest.mark.parametrize("n,W", [(1024, 128), (1000, 128)], ids=str)
@pytest.mark.parametrize("hyst", [64, 256])
def test_position_independence(n, W, hyst):
    """A stream's outputs do not depend on where it sits in the batch: the batch reversed, rotated by 5
    and cut to 1, 15, 16 and 17 streams (unused rows of the 16- and 8-stream workgroups; the helper waves
    pair streams s, s + 11 or s, s + 3, s + 6 and share one quiet flag, so the silent stream meets busy
    partners in both orders).  Every arrangement equals the oracle stream by stream, in both modes."""
    st, exp = Z.streams(n, W, hyst), Z.expected(n, W, hyst)
    want = 2 if (n, W) in Z.DMA_SHAPES else 1
    for fam, bt in st.items():
        B = len(bt.names)
        orders = [list(range(B))[::-1], list(np.roll(np.arange(B), 5)), [0], list(range(min(15, B))),
                  list(range(min(16, B))), list(range(min(17, B)))]
        if fam == "M":
            silent, busy = bt.names.index("silent"), bt.names.index("min_chain")
            orders += [[silent, busy], [busy, silent], [busy] * 11 + [silent], [silent] + [busy] * 11,
                       [busy] * 3 + [silent] + [busy] * 4, [silent] + [busy] * 7]
        for order in orders:
            mag = device_mag(bt.c[np.array(order)])
            for state in (True, False):
                assert plan(n, W, hyst, state) == (want if want != 2 or not state else 3)
                res = launch(mag, bt.params, hyst, state)
                compare(res, exp[fam], bt.names, state, (n, W, hyst, fam, state, order[:6]), order=order)


def test_product_level_events_only_equals_state_mode_and_oracle():
    """detect_zc_preamble_batched on B = 3 one-branch streams of 4096 samples with the default PSS
    reference: want_state=False gives the same mask, counts, events and peak values as want_state=True,
    and both equal the oracle run on the returned corr_mag."""
    rng = np.random.default_rng(2048)
    B, T = 3, 4096
    ref = zc_v2.build_pss_symbol(include_cp=False)
    x = (rng.standard_normal((B, 1, T)) + 1j * rng.standard_normal((B, 1, T))) * 0.3
    x[0, 0, 500:500 + 2048] += ref
    x[1, 0, 1900:1900 + 2048] += ref
    xd = torch.from_numpy(x).cuda()
    a = zc_v2.detect_zc_preamble_batched(xd, want_state=True)
    b = zc_v2.detect_zc_preamble_batched(xd, want_state=False)
    n = T + 2047
    assert plan(n, zc_v2.CORR_WINDOW_SIZE, zc_v2.HYSTERESIS, 0) == 1 and b.state == {} and len(a.state) == 5
    assert torch.equal(a.corr_mag, b.corr_mag)
    assert torch.equal(a.gate_mask, b.gate_mask) and torch.equal(a.n_events, b.n_events)
    for s in range(B):                                      # slots beyond the count are unwritten storage
        k = int(a.n_events[s])
        assert torch.equal(a.events[s, :k], b.events[s, :k]) and torch.equal(a.peak_values[s, :k], b.peak_values[s, :k])
    params = (zc_v2.CORR_WINDOW_SIZE, zc_v2.THRESH_VALUE, zc_v2.THRESH_FRAC_BITS, zc_v2.MIN_CORR_MAG)
    total = 0
    for s in range(B):
        e = Z.run_oracle(b.corr_mag[s].cpu().numpy(), params, zc_v2.HYSTERESIS, reflen=2048)
        k = int(b.n_events[s])
        total += k
        assert k == len(e["events"]) and k <= b.events.shape[1]
        assert np.array_equal(b.events[s, :k].cpu().numpy(), e["events"])
        assert np.array_equal(b.peak_values[s, :k].cpu().numpy(), e["peak_values"])
        assert np.array_equal(b.gate_mask[s].cpu().numpy(), e["gate_mask"].astype(np.uint8))
        for key in ("local_sum", "corr_scaled", "thresh_scaled"):
            assert np.array_equal(a.state[key][s].cpu().numpy(), e[key]), key
        assert np.array_equal(a.state["above_threshold"][s].cpu().numpy(), e["above_threshold"].astype(np.uint8))
    assert total >= 2                                       # the two preambles are detected
