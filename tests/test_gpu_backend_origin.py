"""GPU: the back-end with a stream origin (ofs_rx_backend_at).  A frame cut out of a stream and decoded
with origin = the cut and starts relative to it equals, bit for bit, the same frame decoded inside the
whole resident stream - the generic kernel (n_fft 256) and the fast path (n_fft 1024) alike."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N_BR = 6, 2
KEYS = ("cfo", "h", "xa", "gain", "evm", "evm_db", "slope", "sto")
# (n_fft, cp_len, n_used): the generic kernel, and the register-staged fast path at the synthesized geometry
SHAPES = [(256, 64, 100), (1024, 72, 600)]
CUTS = (0, 1, 37, 999, 1500)                       # 0, odd values, and up to just before the pilot's CP
FAR = (1 << 33) + 5                                # an origin whose sums no longer fit fp32's or an int32's range


def words(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int64)


def same(a: dict, b: dict):
    for k in KEYS:
        assert torch.equal(words(a[k]), words(b[k])), k


@pytest.fixture(scope="module", params=[torch.complex64, torch.complex128], ids=["c64", "c128"])
def setup(request):
    """Streams, known starts and symbols, and per shape the yardstick: the whole stream through
    receiver_backend_batched as it is called today (estimated CFO, and cfo_hz given)."""
    from ofdm_sync_amd import core, synth
    fr = synth.frames_batch(B, n_br=N_BR, snr_db=(15.0, 25.0), seed=5, dtype=request.param)
    ps0 = synth.PRE_PAD + 1024                                    # CP start of the first payload symbol
    rng = np.random.default_rng(3)
    ps = torch.tensor(ps0 + rng.integers(0, 9, B), dtype=torch.int64)           # per-frame starts, odd and even
    case = {}
    for n_fft, cp, U in SHAPES:
        ds = ps + (synth.N_FFT + synth.CYCLIC_PREFIX)
        kw = dict(n_fft=n_fft, cp_len=cp, fs_hz=15.36e6, bins=core.centered_subcarrier_indices(U))
        pil = np.exp(2j * np.pi * rng.random((B, U)))
        dat = np.exp(2j * np.pi * rng.random(U))                  # one row shared by all frames
        cfo = rng.uniform(-4000.0, 4000.0, B)
        ref = core.receiver_backend_batched(fr.x, ps, ds, pil, dat, **kw)
        ref_c = core.receiver_backend_batched(fr.x, ps, ds, pil, dat, cfo_hz=cfo, **kw)
        case[n_fft] = dict(ps=ps, ds=ds, pil=pil, dat=dat, cfo=cfo, kw=kw, ref=ref, ref_c=ref_c)
    torch.cuda.synchronize()
    return fr.x, case


@pytest.mark.parametrize("n_fft", [s[0] for s in SHAPES])
def test_a_slice_with_its_origin_decodes_like_the_whole_stream(setup, n_fft):
    from ofdm_sync_amd import core
    x, case = setup
    c = case[n_fft]
    for s in CUTS:
        xs = x[:, :, s:]
        org = torch.full((B,), s, dtype=torch.int64)
        same(core.receiver_backend_batched(xs, c["ps"] - s, c["ds"] - s, c["pil"], c["dat"], origin=org, **c["kw"]),
             c["ref"])
        same(core.receiver_backend_batched(xs, c["ps"] - s, c["ds"] - s, c["pil"], c["dat"], cfo_hz=c["cfo"],
                                           origin=org, **c["kw"]), c["ref_c"])
    # per-frame cuts, each frame its own origin (frames padded to one length behind their own cut)
    cuts = [0, 1, 37, 999, 1500, 1234]
    T = x.shape[2] - max(cuts)
    xs = torch.stack([x[b, :, s:s + T] for b, s in enumerate(cuts)])
    org = torch.tensor(cuts, dtype=torch.int64)
    same(core.receiver_backend_batched(xs, c["ps"] - org, c["ds"] - org, c["pil"], c["dat"], origin=org, **c["kw"]),
         c["ref"])


@pytest.mark.parametrize("n_fft", [s[0] for s in SHAPES])
def test_far_origins(setup, n_fft):
    """Absolute indices beyond 2^33: the whole array at origin FAR against slices at FAR + s."""
    from ofdm_sync_amd import core
    x, case = setup
    c = case[n_fft]
    far = core.receiver_backend_batched(x, c["ps"], c["ds"], c["pil"], c["dat"], origin=FAR, **c["kw"])
    assert not torch.equal(words(far["h"]), words(c["ref"]["h"]))
    for s in (1, 999):
        same(core.receiver_backend_batched(x[:, :, s:], c["ps"] - s, c["ds"] - s, c["pil"], c["dat"],
                                           origin=FAR + s, **c["kw"]), far)


@pytest.mark.parametrize("n_fft", [s[0] for s in SHAPES])
def test_origin_variants(setup, n_fft):
    from ofdm_sync_amd import core
    x, case = setup
    c = case[n_fft]
    args = (x, c["ps"], c["ds"], c["pil"], c["dat"])
    same(core.receiver_backend_batched(*args, origin=None, **c["kw"]), c["ref"])
    same(core.receiver_backend_batched(*args, origin=torch.zeros(B, dtype=torch.int64), **c["kw"]), c["ref"])
    same(core.receiver_backend_batched(*args, origin=0, cfo_hz=c["cfo"], **c["kw"]), c["ref_c"])
    moved = core.receiver_backend_batched(*args, origin=torch.full((B,), 12345, dtype=torch.int64), **c["kw"])
    assert torch.equal(words(moved["cfo"]), words(c["ref"]["cfo"]))              # the CP correlation ignores it
    assert not torch.equal(words(moved["h"]), words(c["ref"]["h"]))              # the tone's phase does not


def test_the_yardstick_is_finite(setup):
    """Equal words of NaNs would prove little: every yardstick output is a finite number."""
    _, case = setup
    for c in case.values():
        for r in (c["ref"], c["ref_c"]):
            assert all(torch.isfinite(torch.view_as_real(r[k]) if r[k].is_complex() else r[k]).all() for k in KEYS)
