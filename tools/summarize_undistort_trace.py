"""Summary of a rocprofv3 --kernel-trace run of tools/undistort_time.py (its trace_results.db) -> JSON on stdout.

The tool's dispatch order is fixed: per frame size (640x480, 848x480) three cases of nmi_undistort_kernel (frame; frame +
mask; frame + mask with a raw mask), warmup + iters calls each; then three level modes (plain, masked, masked with a hood),
each replaying an undistorted and a distorted level alternately warmup + iters times.  A replay runs from its prep kernel to
the next one.  Warm-up calls and replays are dropped.  Usage: python tools/summarize_undistort_trace.py DB [--iters N --warmup W]
"""
import argparse
import collections
import json
import sqlite3

import numpy as np


def short(name):
    return name.split("(")[0].replace("void ", "").replace("nmi::", "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    n = a.iters + a.warmup
    rows = list(sqlite3.connect(a.db).execute("select name, start, end, duration from kernels order by start"))
    ud = [r for r in rows if "nmi_undistort_kernel" in r[0]]
    out = {"undistort_kernel_us": {}, "level_replays": {}}
    cases = [f"{s} {c}" for s in ("640x480", "848x480") for c in ("frame", "frame+mask", "frame+mask, raw mask")]
    for i, lab in enumerate(cases):
        d = np.array([r[3] for r in ud[i * n:(i + 1) * n][a.warmup:]]) / 1000.0
        out["undistort_kernel_us"][lab] = {"median": round(float(np.median(d)), 2), "min": round(float(d.min()), 2), "max": round(float(d.max()), 2)}
    lv = [r for r in rows if r[1] >= ud[len(cases) * n][1] - 1_000_000]
    starts = [i for i, r in enumerate(lv) if "nmi_level_prep_kernel" in r[0]]
    reps = [lv[p:q] for p, q in zip(starts, starts[1:] + [len(lv)])]
    for m, mode in enumerate(("plain", "masked", "masked_hood")):
        seg = reps[m * 2 * n:(m + 1) * 2 * n]
        for dist in (False, True):
            sel = [ks for ks in seg if any("undistort" in k[0] for k in ks) == dist][a.warmup:]
            per = collections.defaultdict(list)
            for ks in sel:
                for k in ks:
                    per[short(k[0])].append(k[3] / 1000.0)
            out["level_replays"][f"{mode}, {'distorted' if dist else 'undistorted'}"] = {
                "replays": len(sel),
                "span_us": round(float(np.median([(max(k[2] for k in ks) - ks[0][1]) / 1000.0 for ks in sel])), 2),
                "kernel_median_us": {k: round(float(np.median(v)), 2) for k, v in per.items() if len(v) >= len(sel) // 2}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
