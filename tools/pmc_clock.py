"""Per-dispatch duration and SQ_BUSY_CYCLES / ns / 32 (shader clock estimate, GHz) of the aa_fast kernel
from a rocprofv3 --pmc counter_collection.csv, in launch order."""
import collections
import csv
import json
import sys

by = collections.defaultdict(dict)
for r in csv.DictReader(open(sys.argv[1])):
    if "aa_fast_kernel" in r["Kernel_Name"]:
        by[int(r["Dispatch_Id"])][r["Counter_Name"]] = (float(r["Counter_Value"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
dur, ghz, wait = [], [], []
for k in sorted(by):
    c, s, e = by[k]["SQ_BUSY_CYCLES"]
    dur.append(round((e - s) / 1e3, 1))
    ghz.append(round(c / (e - s) / 32, 3))
    wait.append(round(by[k]["SQ_WAIT_ANY"][0] / by[k]["SQ_WAVE_CYCLES"][0], 3))
print(json.dumps({"build": sys.argv[2], "dispatches": len(dur), "duration_us": dur, "busy_cycles_per_ns_per_se": ghz,
                  "wait_any_per_wave_cycle": wait}))
