"""GPU, end to end: chunks in, decoded frames out.  Synthesized streams go in chunks through a chunked
[A][A] detector and ``capture.FrameCapture`` - the triggers are the push's own ``ev_int[:, :, 3]`` /
``n_events``, still on the device - and the captured frames through the back-end with
``origin = start``.  The result equals, bit for bit, the back-end on the whole resident stream at the
``frame_start``s of the one-shot storing detector call (the chunked detector's own yardstick)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N_ANT, L = 6, 2, 128
SYM = 1024 + 72                                    # synth's payload symbol with its CP
F = 2 * L + 2 * SYM                                # preamble + pilot symbol + data symbol
KEYS = ("cfo", "h", "xa", "gain", "evm", "evm_db", "slope", "sto")
CHUNKS = (700, 333, 1024, 511, 97)                 # then the rest of the stream in one final push


def words(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int64)


def _run(dtype):
    from ofdm_sync_amd import _lib, core, synth, sync_aa
    from ofdm_sync_amd.capture import FrameCapture
    quant = dict(full_scale_ratio=1.0) if dtype == torch.int16 else {}
    x = synth.frames_batch(B, preamble_len=2 * L, n_br=N_ANT, n_sym=2, snr_db=(12.0, 20.0), max_offset=200,
                           seed=17, dtype=dtype, **quant).x
    T = x.shape[2]
    # the yardstick's events: ONE storing call on the whole stream
    if dtype == torch.int16:
        one = sync_aa.aa_detect_streaming_batched(x, L=L, outputs=("P", "R", "M"), max_events=8)
        det = sync_aa.AAChunkedDetector(B, N_ANT, L, outputs=(), max_events=8)
    else:
        plan = int(_lib.lib().ofs_aa_plan(_lib.C64, _lib.FP32, N_ANT, T, L))
        assert 1000 <= plan < 1200, plan
        one = sync_aa.aa_detect_streaming_batched(x, L=L, precision="fp32", outputs=("P", "R", "M"), max_events=8)
        det = sync_aa.AAChunkedDetectorF32(B, N_ANT, L, outputs=(), max_events=8)
    n_ev = one.n_events.cpu().tolist()
    ev = one.ev_int.cpu()
    assert max(n_ev) <= 8
    want = [(b, int(ev[b, j, 3])) for b in range(B) for j in range(n_ev[b])
            if ev[b, j, 3] >= 0 and ev[b, j, 3] + F <= T]
    assert {b for b, _ in want} == set(range(B))                  # every stream has a frame to decode
    # history from the gate: a trigger arrives in the push that closes its gate, so frame_start must
    # still be retrievable gate_end - frame_start samples later (the chunk length does not enter)
    H = max(F, int(max(ev[b, j, 2] - ev[b, j, 3] for b in range(B) for j in range(n_ev[b]))) + 1)
    cap = FrameCapture(B, N_ANT, frame_len=F, history=H, max_pending=4, dtype=dtype)

    got_b, got_s, got_f, n = [], [], [], 0
    cuts = list(CHUNKS) + [T - sum(CHUNKS)]
    assert cuts[-1] > 0
    dropped = torch.zeros((B, 3), dtype=torch.int32, device=x.device)
    for i, c in enumerate(cuts):
        fin = i == len(cuts) - 1
        e = det.push(x[:, :, n:n + c], final=fin)
        r = cap.push(x[:, :, n:n + c], e.ev_int[:, :, 3], e.n_events, final=fin)   # device to device
        dropped += r.dropped
        b, _, frames, start = cap.live(r)
        got_b.append(b), got_s.append(start), got_f.append(frames)
        n += c
    gb, gs, gf = torch.cat(got_b), torch.cat(got_s), torch.cat(got_f)
    assert sorted(zip(gb.tolist(), gs.tolist())) == sorted(want)
    # what the capture did not emit is accounted for: starts before the stream, or frames cut by its end
    assert dropped[:, 1].sum().item() == 0
    assert dropped[:, [0, 2]].sum().item() == sum(n_ev) - len(want)

    rng = np.random.default_rng(2)
    pil, dat = np.exp(2j * np.pi * rng.random(600)), np.exp(2j * np.pi * rng.random((len(gb), 600)))
    kw = dict(n_fft=1024, cp_len=72, fs_hz=15.36e6, bins=core.centered_subcarrier_indices(600))
    dec = core.receiver_backend_batched(gf, 2 * L, 2 * L + SYM, pil, dat, origin=gs, **kw)
    ref = core.receiver_backend_batched(x[gb], gs + 2 * L, gs + 2 * L + SYM, pil, dat, **kw)
    for k in KEYS:
        assert torch.equal(words(dec[k]), words(ref[k])), k
    assert torch.isfinite(ref["evm"]).all()
    return len(want)


def test_complex64_streams_through_the_f32_detector():
    assert _run(torch.complex64) >= B


def test_int16_streams_through_the_integer_detector():
    assert _run(torch.int16) >= B
