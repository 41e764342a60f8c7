#!/usr/bin/env python3
"""Per-instantiation rows of fused_layer_ws_kernel from a `rocprofv3 --kernel-trace --stats` output directory:

    python tools/lab/ws_weight_dma_trace.py DIR      # finds DIR/**/*kernel_stats.csv

One line per instantiation (calls, average us, total ms), sorted by name, then the sum over them and over all kernels.
"""
import csv
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ws_resources import label  # noqa: E402


def main():
    files = glob.glob(os.path.join(sys.argv[1], "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        print("no kernel_stats.csv under", sys.argv[1])
        return 1
    rows, total = {}, 0.0
    for r in csv.DictReader(open(files[0])):
        total += float(r["TotalDurationNs"])
        m = re.search(r"fused_layer_ws_kernel<([^>]*)>", r["Name"])
        if m:
            a = tuple({"false": 0, "true": 1}.get(t.strip(), t.strip()) for t in m.group(1).split(","))
            rows[label(tuple(int(v) for v in a))] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e6)
    for k in sorted(rows):
        print("%-42s %5d calls %9.2f us %8.3f ms" % ((k,) + rows[k]))
    ws = sum(v[2] for v in rows.values())
    print("%-42s %27s %8.3f ms" % ("all fused_layer_ws_kernel", "", ws))
    print("%-42s %27s %8.3f ms" % ("all kernels", "", total / 1e6))
    return 0


if __name__ == "__main__":
    sys.exit(main())
