"""Where a FrameCapture.push spends its time, from a rocprofv3 trace of tools/frame_capture_ab.py run with ONE
row (--kinds idle --Tc N, --kinds emit or --kinds sparse): median duration of the gather kernel, of the update kernel, of
the gap between them and of the gap from an update to the next push's gather, over back-to-back pushes
(pairs whose gather starts within 50 us of the previous update's end), and the median device copy.

    rocprofv3 --kernel-trace --memory-copy-trace -d OUT -o fc --output-format csv -- \\
        python tools/frame_capture_ab.py --kinds idle --Tc 1024 --rounds 2
    python tools/frame_capture_kt.py OUT/*/fc_kernel_trace.csv [OUT/*/fc_memory_copy_trace.csv] --tag idle_Tc1024
"""
import argparse
import csv
import json
import statistics


def spans(path, match=None, col="Kernel_Name"):
    rows = [r for r in csv.DictReader(open(path)) if match is None or match in r[col]]
    return sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kernel_trace")
    ap.add_argument("copy_trace", nargs="?")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    g, u = spans(a.kernel_trace, "frame_gather_kernel"), spans(a.kernel_trace, "frame_update_kernel")
    assert len(g) == len(u) and g, (len(g), len(u))
    med = lambda v: round(statistics.median(v) / 1e3, 2) if v else None  # noqa: E731
    chained = [i for i in range(1, len(g)) if 0 <= g[i][0] - u[i - 1][1] < 50_000]
    out = dict(tool="frame_capture_kt", tag=a.tag, pushes=len(g), chained=len(chained),
               gather_us=med([g[i][1] - g[i][0] for i in chained]), update_us=med([u[i][1] - u[i][0] for i in chained]),
               gap_gather_to_update_us=med([u[i][0] - g[i][1] for i in chained]),
               gap_update_to_next_gather_us=med([g[i][0] - u[i - 1][1] for i in chained]),
               push_period_us=med([g[i][0] - g[i - 1][0] for i in chained]))
    if a.copy_trace:
        c = spans(a.copy_trace)
        dur = [e - s for s, e in c]
        big = [d for d in dur if d >= 0.5 * max(dur)]                # the chunk copies (the tool's small ones aside)
        out.update(copies=len(big), copy_us=med(big))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
