"""Summary of a rocprofv3 --kernel-trace --output-format csv run of tools/deep_time.py (its *_kernel_trace.csv) -> JSON on stdout.
The tool's phases run one after the other, REPLAYS level replays each, and a replay ends with its search kernel (nmi_grid_kernel
or nmi_pix_kernel), so the dispatches are cut into phases after every REPLAYS-th search dispatch; per phase, the median duration of
every kernel that ran at least once per two replays (the tone table kernel a fixed mode launches once, at its setting, is listed
under `once`).  PHASES names them, comma-separated, in the tool's order (default: numbered).
Usage: python tools/summarize_deep_trace.py TRACE.csv REPLAYS [PHASES]"""
import collections
import csv
import json
import re
import sys

import numpy as np


def short(name):
    m = re.search(r"(nmi_\w+?)(<.*)?\(", name + "(")
    base = m.group(1) if m else name
    t = re.search(r"nmi_gray16_kernel<(\d), (true|false|\(bool\)[01])", name)  # <F, Masked, ...>
    if t:
        return f"nmi_gray16{'_masked' if t.group(2) in ('true', '(bool)1') else ''}_kernel<{t.group(1)}>"
    return base


def main():
    replays = int(sys.argv[2])
    names = sys.argv[3].split(",") if len(sys.argv) > 3 else None
    with open(sys.argv[1]) as f:
        rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)))
    phases, cur, searches = [], collections.defaultdict(list), 0
    for t0, t1, name in rows:
        k = short(name)
        cur[k].append((t1 - t0) / 1e3)
        if re.fullmatch(r"nmi_(grid|pix)_kernel", k):
            searches += 1
            if searches == replays:
                phases.append(cur)
                cur, searches = collections.defaultdict(list), 0
    out = []
    for i, ph in enumerate(phases):
        per_replay = {k: round(float(np.median(v)), 2) for k, v in sorted(ph.items()) if len(v) * 2 >= replays}
        once = {k: [round(x, 2) for x in v] for k, v in sorted(ph.items()) if len(v) * 2 < replays and k.startswith("nmi_tone")}
        out.append({"phase": names[i] if names and i < len(names) else i, "median_us": per_replay, "once": once})
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
