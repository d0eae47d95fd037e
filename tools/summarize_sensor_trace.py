"""Summary of a rocprofv3 --kernel-trace --output-format csv run of tools/sensor_time.py (its *_kernel_trace.csv) -> JSON on stdout:
median / min / max duration of the conversion kernels (nmi_gray_kernel<C, R>: C bytes per pixel, R the byte of red or of luma;
nmi_bayer_kernel<F>: a mosaic at factor F) and of the undistortion kernel's instantiations (GrayTaps: a grey frame;
ColorTaps<C, R>, BayerTaps: the fused nodes), per grid (848x480 frames are a 256 x 480 grid, 1241x376 ones 320 x 376).  Every
dispatch counts, warm-up ones included.  With PASSES > 1 each kernel's dispatches, in the order they ran, are also split into
that many equal parts -- the --repeats passes of the tool -- and the medians of the parts are listed: their spread is how far a
median moves within one session.
Usage: python tools/summarize_sensor_trace.py TRACE.csv [PASSES]"""
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
    m = re.search(r"nmi_bayer_kernel<(\d)>", name)
    if m:
        return f"bayer_kernel<{m.group(1)}>"
    m = re.search(r"nmi_undistort_kernel<[^>]*?(GrayTaps|BayerTaps|ColorTaps<(\d), (\d)>)", name)
    if m:
        return f"undistort_kernel<{m.group(1) if m.group(2) is None else f'ColorTaps<{m.group(2)},{m.group(3)}>'}>"
    return None


def main():
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    d = collections.defaultdict(list)
    with open(sys.argv[1]) as f:
        for r in csv.DictReader(f):
            lab = label(r["Kernel_Name"])
            if lab:
                d[f"{lab} grid {r['Grid_Size_X']}x{r['Grid_Size_Y']}"].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    out = {}
    for k, v in sorted(d.items()):
        us = [t for _, t in sorted(v)]
        out[k] = {"n": len(us), "median_us": round(float(np.median(us)), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}
        if passes > 1 and len(us) >= passes:
            parts = [round(float(np.median(p)), 2) for p in np.array_split(np.array(us), passes)]
            out[k]["pass_medians_us"] = parts
            out[k]["pass_spread_us"] = round(max(parts) - min(parts), 2)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
