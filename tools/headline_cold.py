"""bench.py's timed region on the headline detector (cfg3: 65536 x 1024 c64, L = 512, P/R/M + events) in a
fresh process under debug variants: synthesis, 10 warm-up launches, 100 timed ones - the first launches
after other work, not the settled state tools/headline_ab.py measures.  Diagnostic tooling (not the product).

    python tools/headline_cold.py [K=V[,K2=V2]]      (ofs_debug_set_variant names; none: default dispatch)

Run the arms in alternating processes; prints one JSON line.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ofdm-sync-math_amd"))
from ofdm_sync_amd import _lib, synth, sync_aa  # noqa: E402


def main():
    vs = dict(kv.split("=") for kv in sys.argv[1].split(",") if kv) if len(sys.argv) > 1 else {}
    dev = torch.device("cuda", 0)
    det = sync_aa.AABatchDetector(65536, 1024, 1, 512, outputs=("P", "R", "M"), max_events=4, device=dev)
    det.x.copy_(synth.headline_batch(65536, 1024, 512, seed=2026, device=dev))
    torch.cuda.empty_cache()
    for k, v in vs.items():
        _lib.set_variant(k, int(v))
    st = torch.cuda.current_stream()
    for _ in range(10):
        det.run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(100):
        det.run()
    e1.record(st)
    torch.cuda.synchronize()
    print(json.dumps({"variants": vs, "ms_per_step": round(e0.elapsed_time(e1) / 100, 5)}), flush=True)


if __name__ == "__main__":
    main()
