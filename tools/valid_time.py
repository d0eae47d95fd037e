"""Valid-range timing (nmi_set_valid_range on GRAY16 frames), after tools/clahe_time.py.  Prints one JSON line.

Phases, one after the other, host wall time of each call (the call ending in a synchronise):
  off/<size>/<content>/<mode>    nmi_gray_frame of a 640x480 frame, nmi_reduce_frame of a 2560x1920 source at factor 4, range off:
                                 content thermal (a 14-bit band 7000 .. 7400, twenty pixels at 16383; bits 14) or uniform (noise
                                 over 16 bits; bits 16); mode equalize or clahe (8 x 8 tiles).  These run on any library with
                                 CLAHE, so an earlier commit's (through NMI_HIP_LIBRARY) can be timed beside this one's.
  on/<size>/<content>/<mode>     the same calls with a range on (thermal: (0, 16382), the hot pixels out; uniform: (4096, 61439))
  deep/<size>/<content>/<mode>   nmi_deep_frame under that range: the masked conversion, with a frame mask
The on and deep phases need a library with nmi_set_valid_range and are skipped on one without.

Kernel times: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/valid_time.py --iters 100 (every phase, so the
unranged kernels stand beside the ranged ones; --range-only leaves the off phases out), then python
tools/summarize_clahe_trace.py TRACE.csv CALLS_PER_PHASE PHASES (both printed in the JSON line).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbslam2_nmi_amd as nmi  # noqa: E402
from clahe_time import contents, med  # noqa: E402
from orbslam2_nmi_amd import capi  # noqa: E402

W, H = 640, 480
GRAY16 = capi.FRAME_GRAY16
RANGES = {"thermal": (0, 16382), "uniform": (4096, 61439)}


def modes(bits):
    return {"equalize": capi.ToneMap.equalize(0, bits), "clahe": capi.ToneMap.clahe(8, 8, 0, bits)}


def timed(call, iters, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"call_us": med(ts), "p10_us": round(float(np.percentile(ts, 10)), 2), "p90_us": round(float(np.percentile(ts, 90)), 2)}


def frame_phases(ctx, res, a, ranged):
    out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    out_mask = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    fm = torch.ones((H, W), dtype=torch.uint8, device="cuda")
    fm[H - H // 6:] = 0
    for f in (1, 4):
        for cname, (px, bits) in contents(f * W, f * H).items():
            src = torch.from_numpy(np.ascontiguousarray(px).view(np.uint8).reshape(-1)).cuda()
            for mname, tm in modes(bits).items():
                ctx.set_tone_map(tm)

                def call():
                    if f == 1:
                        ctx.gray_frame(src, GRAY16, 0, out=out)
                    else:
                        ctx.reduce_frame(src, GRAY16, f, 0, out=out)

                def deep():
                    ctx.deep_frame(src, f, 0, frame_mask=fm, out=out, out_mask=out_mask)

                todo = [("off", call, None)] if not a.range_only else []
                if ranged:
                    todo += [("on", call, RANGES[cname]), ("deep", deep, RANGES[cname])]
                for kind, fn, rng in todo:
                    if ranged:
                        ctx.set_valid_range(*(rng or (0, 65535)))
                    ph = timed(fn, a.iters, a.warmup)
                    ph["name"] = f"{kind}/{f * W}x{f * H}/{cname}/{mname}"
                    ph["checksum"] = int(out.sum().item())
                    res["phases"].append(ph)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--range-only", action="store_true", help="the on and deep phases alone (kernel traces)")
    a = ap.parse_args()
    lib = capi.load_library()
    ranged = hasattr(lib, "nmi_set_valid_range")
    res = {"shape": [W, H], "calls_per_phase": a.iters + a.warmup, "valid_range": ranged, "phases": []}
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    with nmi.NmiContext(W, H) as ctx:
        ctx.set_stream(st.cuda_stream)
        frame_phases(ctx, res, a, ranged)
    torch.cuda.set_stream(torch.cuda.default_stream())
    res["phase_names"] = ",".join(p["name"] for p in res["phases"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
