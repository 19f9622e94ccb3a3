#!/usr/bin/env python3
"""Run tests/test_gpu_backend_exact.py on the GPU and print, as a markdown table, the worst deviation each frame
family left on each output of each kernel beside its tolerance (profiles/backend_exact_margins.md).

    python tools/backend_margins.py profiles/backend_exact_margins.md
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_gpu_backend_exact.py")])
    mod = sys.modules.get("test_gpu_backend_exact")
    if mod is None:
        return int(rc) or 1
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    keys = ("cfo", "h", "xa", "gain", "evm", "evm_db", "slope", "sto")
    print("# Back-end exact frames: worst deviation against the model, per family, kernel and output\n", file=out)
    print("Each cell: worst absolute deviation / its tolerance (the frame with the largest ratio), over every shape,", file=out)
    print("bin set, branch count and input format of tests/test_gpu_backend_exact.py.  `delay_closed` is the delay", file=out)
    print("family against the closed forms instead of the model.  pytest exit code: %d.\n" % int(rc), file=out)
    print("| family | kernel | " + " | ".join(keys) + " |", file=out)
    print("|---|---|" + "---|" * len(keys), file=out)
    for fam, kern in sorted({(f, k) for f, k, _ in mod.MARGINS}):
        cells = ["%.2g / %.2g" % tuple(mod.MARGINS[(fam, kern, key)]) for key in keys]
        print(f"| {fam} | {kern} | " + " | ".join(cells) + " |", file=out)
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
