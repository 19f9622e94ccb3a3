"""Per-dispatch durations (us, launch order) of the aa_fast kernel from a rocprofv3 kernel_trace.csv."""
import csv
import json
import sys

rows = [r for r in csv.DictReader(open(sys.argv[1])) if "aa_fast_kernel" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
d = [round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, 2) for r in rows]
gaps = [round((int(b["Start_Timestamp"]) - int(a["End_Timestamp"])) / 1e3, 2) for a, b in zip(rows, rows[1:])]
s = sorted(d)
print(json.dumps({"build": sys.argv[2], "kernel": rows[0]["Kernel_Name"], "calls": len(d), "avg_us": round(sum(d) / len(d), 2),
                  "min_us": s[0], "median_us": s[len(s) // 2], "max_us": s[-1], "median_gap_us": sorted(gaps)[len(gaps) // 2],
                  "durations_us": d}))
