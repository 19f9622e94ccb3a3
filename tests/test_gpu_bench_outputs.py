"""GPU: bench.py's plain run and --dump-outputs on a small batch (in process, one launch shape).

A plain run prints the headline line without the --full legs; --dump-outputs writes the last
timed step's results as float32 / float64 .npy files that repeat bit for bit from run to run
and equal what a caller of ``AABatchDetector.run`` on the same seeded input receives."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("needs a GPU", allow_module_level=True)

pytestmark = pytest.mark.gpu

B, T, L = 3000, 1024, 512                  # > bench.DUMP_ROWS streams: the seeded row sample is exercised
NAMES = ("rows", "P", "R", "M", "n_events", "ev_int", "ev_real")


def _run(capsys, out_dir, *extra):
    import bench
    assert bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B), "--dump-outputs",
                       str(out_dir), *extra]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {n: np.load(os.path.join(out_dir, n + ".npy")) for n in NAMES}


def test_plain_run_dumps_last_step_outputs(capsys, tmp_path):
    import bench
    from ofdm_sync_amd import shard, sync_aa, synth
    r, a = _run(capsys, tmp_path / "a")
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(B * T / (r["ms_per_step"] / 1e3) / 1e6, rel=1e-3)
    assert r["cpu_baseline"] is None and "parity" not in r          # those legs run under --full only
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in NAMES)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    rows = a["rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and np.all(np.diff(rows) > 0) and rows[-1] < B
    # a second run: same inputs, same outputs
    _, b = _run(capsys, tmp_path / "b")
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
    # the same seeded batch through the product API
    dev = torch.device("cuda", 0)
    det = sync_aa.AABatchDetector(B, T, 1, L, precision="fp32", outputs=("P", "R", "M"), max_events=4, device=dev)
    det.x.copy_(synth.headline_batch(B, T, L, seed=shard.shard_seed(2026, 0), device=dev))
    res = det.run()
    torch.cuda.synchronize()
    assert np.array_equal(a["P"], torch.view_as_real(res.P).cpu().numpy()[rows])
    assert np.array_equal(a["R"], res.R.cpu().numpy()[rows])
    assert np.array_equal(a["M"], res.M.cpu().numpy()[rows])
    assert np.array_equal(a["n_events"], res.n_events.cpu().numpy())
    assert np.array_equal(a["ev_int"], res.ev_int.cpu().numpy())
    assert np.array_equal(a["ev_real"], res.ev_real.cpu().numpy())
    assert a["n_events"].sum() > 0.5 * B                            # the batch contains detections
