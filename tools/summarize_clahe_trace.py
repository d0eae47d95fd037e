"""Summary of a rocprofv3 --kernel-trace --output-format csv run of tools/clahe_time.py (its *_kernel_trace.csv) -> JSON on stdout.
The tool's phases run one after the other, CALLS conversions each, and a conversion ends with its conversion kernel
(nmi_gray16_kernel<F, Masked> or nmi_clahe_gray16_kernel<F, Masked>; the masked ones: tools/valid_time.py), so the dispatches are cut into phases after every CALLS-th such dispatch;
per phase, the median duration of every nmi_* kernel that ran at least once per two calls, and their sum.  PHASES names them,
comma-separated, in the tool's order (its "phase_names").  The masked conversions (<F, true, ...>) and the ranged histograms
(<true, ...>) are listed as nmi_*gray16_masked_kernel<F> and nmi_*_hist_ranged_kernel, the plain ones as nmi_*gray16_kernel<F> and
nmi_*_hist_kernel: the labels of the summaries under profiles/.
Usage: python tools/summarize_clahe_trace.py TRACE.csv CALLS [PHASES]"""
import collections
import csv
import json
import re
import sys

import numpy as np


ON = r"(true|false|\(bool\)[01])"


def short(name):
    m = re.search(r"(nmi_(?:clahe_)?gray16)_kernel<(\d), " + ON, name)
    if m:
        return f"{m.group(1)}{'_masked' if m.group(3) in ('true', '(bool)1') else ''}_kernel<{m.group(2)}>"
    m = re.search(r"(nmi_(?:tone|clahe)_hist)_kernel<" + ON, name)
    if m:
        return f"{m.group(1)}{'_ranged' if m.group(2) in ('true', '(bool)1') else ''}_kernel"
    m = re.search(r"(nmi_\w+?)(<(\d)>)?\(", name + "(")
    if not m:
        return name
    return f"{m.group(1)}<{m.group(3)}>" if m.group(3) else m.group(1)


def main():
    calls = int(sys.argv[2])
    names = sys.argv[3].split(",") if len(sys.argv) > 3 else None
    with open(sys.argv[1]) as f:
        rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)))
    phases, cur, done = [], collections.defaultdict(list), 0
    for t0, t1, name in rows:
        k = short(name)
        if not k.startswith("nmi_"):
            continue
        cur[k].append((t1 - t0) / 1e3)
        if re.fullmatch(r"nmi_(clahe_)?gray16(_masked)?_kernel<\d>", k):
            done += 1
            if done == calls:
                phases.append(cur)
                cur, done = collections.defaultdict(list), 0
    out = []
    for i, ph in enumerate(phases):
        per_call = {k: round(float(np.median(v)), 2) for k, v in sorted(ph.items()) if len(v) * 2 >= calls}
        out.append({"phase": names[i] if names and i < len(names) else i, "median_us": per_call, "sum_us": round(sum(per_call.values()), 2)})
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
