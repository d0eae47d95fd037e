"""Summary of a rocprofv3 --kernel-trace --output-format csv run of tools/packed_time.py --kernels-only (its *_kernel_trace.csv) ->
JSON on stdout: per kernel and grid size (the tool unpacks two source sizes with the same kernels), the number of dispatches
and their median, 10th and 90th percentile duration in us.  Kernels of the device-to-device copy, where the runtime
dispatches one, are listed under the name it gives them.
Usage: python tools/summarize_packed_trace.py TRACE.csv"""
import collections
import csv
import json
import sys

import numpy as np


def main():
    groups = collections.defaultdict(list)
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            grid = [int(r.get(f"Grid_Size_{a}", 0) or 0) for a in "XYZ"]
            groups[(r["Kernel_Name"], tuple(grid))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = [{"kernel": k, "grid": list(g), "dispatches": len(v), "median_us": round(float(np.median(v)), 2),
            "p10_us": round(float(np.percentile(v, 10)), 2), "p90_us": round(float(np.percentile(v, 90)), 2)}
           for (k, g), v in sorted(groups.items())]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
