"""Summary of a rocprofv3 --kernel-trace --output-format csv run of tools/reduce_time.py --part kernel (its *_kernel_trace.csv) ->
JSON on stdout.  Per kernel and grid: the dispatches in time order, the warm-up ones dropped, split into the tool's rounds;
median of each round, their min and max (the run-to-run spread of that measurement), and the median over all rounds.  Kernels:
nmi_reduce_kernel<C, R, F, mask> (C bytes per pixel, R the byte of red, F the factor) and nmi_gray_kernel<C, R> on the same
full-size sources.  Then the bar of each pair: the reduction's median may exceed the full-size conversion's by no more than the
conversion's own spread.
Usage: python tools/summarize_reduce_trace.py TRACE.csv [--rounds 6] [--iters 200]"""
import argparse
import collections
import csv
import json
import re

import numpy as np

# (reduction, full-size conversion) as "label grid" prefixes; grids are in threads: 64 lanes x ceil(runs / 64), rows rounded up to 4
PAIRS = {
    "1920x1080 RGB -> 960x540": ("reduce_kernel<3,0,2>", "gray_kernel<3,0> grid 512x1080"),
    "3840x2160 BGRA -> 960x540": ("reduce_kernel<4,2,4>", "gray_kernel<4,2> grid 960x2160"),
}


def label(name):
    m = re.search(r"nmi_reduce_kernel<(\d+), (\d+), (\d+), (false|true|0|1)>", name)
    if m:
        return f"reduce_kernel<{m.group(1)},{m.group(2)},{m.group(3)}>" + ("" if m.group(4) in ("false", "0") else " mask")
    m = re.search(r"nmi_gray_kernel<(\d+), (\d+)>", name)
    if m:
        return f"gray_kernel<{m.group(1)},{m.group(2)}>"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    d = collections.defaultdict(list)
    with open(a.trace) as f:
        for r in csv.DictReader(f):
            lab = label(r["Kernel_Name"])
            if lab:
                d[f"{lab} grid {r['Grid_Size_X']}x{r['Grid_Size_Y']}"].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    out = {}
    for k, v in sorted(d.items()):
        us = [t for _, t in sorted(v)][-a.rounds * a.iters:]
        rounds = [us[i * a.iters:(i + 1) * a.iters] for i in range(len(us) // a.iters)] or [us]
        meds = [round(float(np.median(r)), 3) for r in rounds]
        out[k] = {"n": len(us), "round_medians_us": meds, "min_round_us": min(meds), "max_round_us": max(meds),
                  "spread_us": round(max(meds) - min(meds), 3), "median_us": round(float(np.median(us)), 3)}
    bars = {}
    for name, (red, gray) in PAIRS.items():
        r = [v for k, v in out.items() if k.startswith(red)]
        g = [v for k, v in out.items() if k.startswith(gray)]
        if len(r) == 1 and len(g) == 1:
            bars[name] = {"reduce_median_us": r[0]["median_us"], "gray_full_size_median_us": g[0]["median_us"], "gray_spread_us": g[0]["spread_us"],
                          "holds": r[0]["median_us"] <= g[0]["median_us"] + g[0]["spread_us"]}
    print(json.dumps({"kernels": out, "bar": bars}, indent=1))


if __name__ == "__main__":
    main()
