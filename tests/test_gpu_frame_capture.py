"""GPU: ofs_frame_capture_chunk / capture.FrameCapture against slices of the whole stream and the
bookkeeping of the plain-Python model (tests/capture_model.py), bit for bit, for every chunking."""

import numpy as np
import pytest
import torch

import capture_model as cm

pytestmark = pytest.mark.gpu

KINDS = {"c64": torch.complex64, "c128": torch.complex128, "i16": torch.int16}
PATTERN = 0x5A                                                    # byte of the pre-filled frame buffer


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's words as integers (CPU)."""
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().cpu().view(torch.uint8)


def run_gpu(sc: cm.Scenario, chunks, x: np.ndarray, kind: str, strided: bool = True):
    """One scenario through FrameCapture.  Before every push the frame buffer is filled with PATTERN;
    after it the four outputs are cloned on the device; everything is compared at the end.  Returns
    per stream the list of starts in the order they came out."""
    from ofdm_sync_amd.capture import FrameCapture
    n_br = x.shape[1]
    cap = FrameCapture(cm.B, n_br, frame_len=sc.F, history=sc.H, max_pending=sc.Q, offset=sc.offset,
                       dtype=KINDS[kind])
    xd = torch.from_numpy(x).cuda()
    dl = cm.deliveries(sc, chunks)
    want = cm.run_model(sc, chunks, x)
    got, n = [], 0
    pushes = list(enumerate(chunks)) + ([(None, 0)] if sc.flush else [])
    for p, c in pushes:
        if p is not None and p in sc.resets:
            mask = torch.zeros(cm.B, dtype=torch.bool)
            mask[sc.resets[p]] = True
            cap.reset(mask)
        bits_view = cap._res.frames.view(torch.uint8) if kind == "i16" else torch.view_as_real(cap._res.frames).view(torch.uint8)
        bits_view.fill_(PATTERN)
        if p is None:
            r = cap.flush()
        else:
            K = max(1, max(len(v) for v in dl[p]))
            ev = np.full((cm.B, K, 4), -(1 << 40), dtype=np.int64)               # a padding value is always late
            cnt = np.zeros(cm.B, dtype=np.int32)
            for b, vals in enumerate(dl[p]):
                ev[b, :len(vals), 3] = vals
                cnt[b] = len(vals) + (sc.over_count if len(vals) == K else 0)
            evd = torch.from_numpy(ev).cuda()
            starts = evd[:, :, 3] if strided else evd[:, :, 3].contiguous()
            if any(dl[p]) or sc.over_count:
                r = cap.push(xd[:, :, n:n + c], starts, torch.from_numpy(cnt).cuda(),
                             final=sc.final and p == len(chunks) - 1)
            else:                                                 # no trigger anywhere: the plain form
                r = cap.push(xd[:, :, n:n + c], final=sc.final and p == len(chunks) - 1)
            n += c
        got.append((r.frames.clone(), r.frame_start.clone(), r.n_frames.clone(), r.dropped.clone()))
    torch.cuda.synchronize()
    order = {b: [] for b in range(cm.B)}
    pat = None
    for i, ((fr, fs, nf, dr), out) in enumerate(zip(got, want)):
        fr, fs, nf, dr = fr.cpu(), fs.cpu(), nf.cpu(), dr.cpu()
        if pat is None:
            pat = torch.full_like(bits(fr[0, 0]), PATTERN)
        for b, (starts, frames, dropped) in enumerate(out):
            tag = (sc.name, kind, n_br, i, b)
            assert nf[b].item() == len(starts), tag
            assert fs[b].tolist() == starts + [-1] * (sc.Q - len(starts)), tag
            assert dr[b].tolist() == dropped, tag
            for slot in range(sc.Q):
                if slot < len(starts):
                    assert torch.equal(bits(fr[b, slot]), bits(torch.from_numpy(np.ascontiguousarray(frames[slot])))), (tag, slot)
                    if not sc.resets:                             # the model's frame IS the slice (host test); again here
                        s = starts[slot]
                        assert torch.equal(bits(fr[b, slot]), bits(torch.from_numpy(np.ascontiguousarray(x[b, :, s:s + sc.F])))), (tag, slot)
                else:
                    assert torch.equal(bits(fr[b, slot]), pat), (tag, slot, "unused slot written")
            order[b] += starts
    return order


@pytest.mark.parametrize("n_br", [1, 2])
@pytest.mark.parametrize("kind", list(KINDS))
def test_any_chunking_gives_the_same_frames(kind, n_br):
    total = 0
    for F, H in cm.SIZES:
        sc = cm.clean_scenario(F, H)
        x = cm.make_stream(kind, n_br, sc.T, seed=F + H)
        want = {b: [val + sc.offset for bb, val, _ in sc.triggers if bb == b] for b in range(cm.B)}
        for name, chunks in cm.chunkings(sc.T, F, H).items():
            assert run_gpu(sc, chunks, x, kind) == want, (F, H, name)
            total += 1
    assert total == 4 * len(cm.SIZES) + 1                         # + the one-sample pushes of the smallest F, H


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("sc", cm.edge_scenarios(), ids=lambda s: s.name)
def test_edges(sc, kind):
    for n_br in (1, 2):
        x = cm.make_stream(kind, n_br, sc.T, seed=7)
        order = run_gpu(sc, sc.chunks, x, kind)
        assert sum(len(v) for v in order.values()) > 0


@pytest.mark.parametrize("kind", list(KINDS))
def test_strided_triggers_equal_the_contiguous_copy(kind):
    sc = cm.clean_scenario(7, 44)
    x = cm.make_stream(kind, 2, sc.T, seed=3)
    chunks = cm.chunkings(sc.T, 7, 44)["primes"]
    assert run_gpu(sc, chunks, x, kind, strided=True) == run_gpu(sc, chunks, x, kind, strided=False)


def test_all_K_when_n_starts_is_none():
    from ofdm_sync_amd.capture import FrameCapture
    x = torch.from_numpy(cm.make_stream("c64", 1, 64)).cuda()
    cap = FrameCapture(cm.B, 1, frame_len=5, history=9, max_pending=3)
    st = torch.tensor([[3, 40, 0]] * cm.B, dtype=torch.int64).cuda()
    r = cap.push(x[:, 0, :32], st)                                # [B, Tc] for one branch
    b, slot, frames, start = cap.live(r)
    assert b.tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] and slot.tolist() == [0, 1] * cm.B
    assert start.tolist() == [3, 0] * cm.B and tuple(frames.shape) == (10, 1, 5)
    assert torch.equal(bits(frames[2]), bits(x[1, :, 3:8])) and torch.equal(bits(frames[3]), bits(x[1, :, 0:5]))
    r = cap.push(x[:, 0, 32:])
    assert cap.live(r)[3].tolist() == [40] * cm.B and r.dropped.sum().item() == 0


# ---------------------------------------------------------------------------------------------
# argument refusals at the C ABI: the error status, and nothing launched (state and outputs untouched)
# ---------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    from ofdm_sync_amd import _lib
    lib = _lib.lib()
    B, nb, F, H, Q, Tc = 3, 1, 8, 8, 2, 16
    nbytes = lib.ofs_frame_capture_state_bytes(_lib.C64, nb, F, H, Q)
    assert nbytes > 0 and nbytes % 16 == 0 and nbytes >= nb * H * 8
    for bad in ((_lib.C64, nb, F, F - 1, Q), (_lib.C64, nb, F, H, 0), (_lib.C64, nb, F, H, 17), (_lib.CP12, nb, F, H, Q),
                (7, nb, F, H, Q), (_lib.C64, 0, F, H, Q), (_lib.C64, nb, 0, H, Q)):
        assert lib.ofs_frame_capture_state_bytes(*bad) < 0, bad
    assert getattr(lib, "ofs_frame_capture_max_samples", None) is None          # no chunk limit, no such function
    state = torch.full((B, nbytes), 0x33, dtype=torch.uint8, device="cuda")
    x = torch.zeros((B, nb, Tc), dtype=torch.complex64, device="cuda")
    frames = torch.full((B, Q, nb, F, 2), 7.0, dtype=torch.float32, device="cuda")
    fs = torch.full((B, Q), 99, dtype=torch.int64, device="cuda")
    nf = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    dr = torch.full((B, 3), 99, dtype=torch.int32, device="cuda")
    trig = torch.zeros((B, 1), dtype=torch.int64, device="cuda")
    ntr = torch.ones((B,), dtype=torch.int32, device="cuda")
    before = [t.clone() for t in (state, frames, fs, nf, dr)]

    def call(fmt=_lib.C64, xp=x.data_ptr(), Tc=Tc, F=F, H=H, Q=Q, sp=state.data_ptr(), final=0, trig_max=1, nb=nb):
        return lib.ofs_frame_capture_chunk(fmt, xp, B, nb, Tc, F, H, Q, 0, trig.data_ptr(), 1, 1, ntr.data_ptr(),
                                           trig_max, sp, frames.data_ptr(), fs.data_ptr(), nf.data_ptr(),
                                           dr.data_ptr(), final, _lib.stream_ptr())
    EINVAL = -1
    assert call(H=F - 1) == EINVAL                                # history < frame_len
    assert call(Q=0) == EINVAL and call(Q=17) == EINVAL           # max_pending
    assert call(fmt=_lib.CP12) == EINVAL and call(fmt=9) == EINVAL and call(fmt=-1) == EINVAL
    assert call(sp=state.data_ptr() + 8) == EINVAL                # unaligned state
    assert call(sp=None) == EINVAL
    assert call(Tc=0) == EINVAL                                   # empty chunk without final
    assert call(xp=None) == EINVAL and call(Tc=-1) == EINVAL and call(F=0) == EINVAL and call(nb=0) == EINVAL
    assert call(trig_max=-1) == EINVAL
    torch.cuda.synchronize()
    for t, b4 in zip((state, frames, fs, nf, dr), before):
        assert torch.equal(t, b4)
    # ... and the same arguments without the fault are taken (fresh state)
    state.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert nf.tolist() == [1] * B and fs[:, 0].tolist() == [0] * B and dr.sum().item() == 0


def test_python_refusals():
    from ofdm_sync_amd.capture import FrameCapture
    with pytest.raises(ValueError):
        FrameCapture(2, 1, frame_len=8, history=7)
    with pytest.raises(ValueError):
        FrameCapture(2, 1, frame_len=8, max_pending=17)
    with pytest.raises(ValueError):
        FrameCapture(2, 1, frame_len=8, dtype=torch.float32)
    cap = FrameCapture(2, 1, frame_len=8)
    assert cap.history == 8 and cap.max_chunk is None
    x = torch.zeros((2, 1, 4), dtype=torch.complex64, device="cuda")
    with pytest.raises(ValueError):
        cap.push(x[:, :, :0])                                     # empty chunk without final
    with pytest.raises(ValueError):
        cap.push(x, torch.zeros((2, 1), dtype=torch.int32, device="cuda"))      # starts must be int64
    with pytest.raises(ValueError):
        cap.push(x.to(torch.complex128))
