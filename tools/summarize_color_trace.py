"""Summary of a rocprofv3 --kernel-trace --output-format csv run of tools/color_time.py (its *_kernel_trace.csv) -> JSON on stdout:
median / min / max duration of the conversion kernels (nmi_gray_kernel<C, R>: C bytes per pixel, R the byte of red) and of the
undistortion kernel's instantiations (GrayTaps: a grey frame; ColorTaps<C, R>: the fused colour node), per grid (848x480 frames
are a 256 x 480 grid, 1241x376 ones 320 x 376).  Every dispatch counts, warm-up ones included (the kernels do not change with it).
Usage: python tools/summarize_color_trace.py TRACE.csv"""
import collections
import csv
import json
import re
import sys

import numpy as np


def label(name):
    m = re.search(r"nmi_gray_kernel<(\d), (\d)>", name)
    if m:
        return f"gray_kernel<{m.group(1)},{m.group(2)}>"
    m = re.search(r"nmi_undistort_kernel<[^>]*?(GrayTaps|ColorTaps<(\d), (\d)>)", name)
    if m:
        return "undistort_kernel<GrayTaps>" if m.group(1) == "GrayTaps" else f"undistort_kernel<ColorTaps<{m.group(2)},{m.group(3)}>>"
    return None


def main():
    d = collections.defaultdict(list)
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            lab = label(r["Kernel_Name"])
            if lab:
                d[f"{lab} grid {r['Grid_Size_X']}x{r['Grid_Size_Y']}"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {k: {"n": len(v), "median_us": round(float(np.median(v)), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for k, v in sorted(d.items())}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
