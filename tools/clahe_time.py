"""CLAHE timing (NMI_TONE_CLAHE beside NMI_TONE_EQUALIZE on GRAY16 frames), after tools/deep_time.py.  Prints one JSON line.

nmi_gray_frame of a 640x480 frame, and nmi_reduce_frame of a 2560x1920 source at factor 4 into the same 640x480 context: host
wall time of each call, the call ending in a synchronise, in phases that run one after the other:
  <size>/<content>/<mode>   content thermal (a 14-bit band 7000 .. 7400 around a scene, twenty pixels at 16383; bits 14) or
                            uniform (noise over 16 bits; bits 16); mode equalize, clahe (8 x 8 tiles, no plateau) or clahe-p4
                            (plateau 4)
A library without CLAHE (an earlier commit's, through NMI_HIP_LIBRARY) runs the equalize phases alone.

Kernel times: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/clahe_time.py --iters 100, then
python tools/summarize_clahe_trace.py TRACE.csv CALLS_PER_PHASE PHASES (both printed in the JSON line).
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
from orbslam2_nmi_amd import capi  # noqa: E402

W, H = 640, 480
GRAY16 = 48


def scene(w, h, seed=0):
    """A smooth 8-bit scene with texture: blobs and a gradient."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = 60 + 100 * x / w + 40 * np.sin(y / 37.0) * np.cos(x / 53.0)
    for _ in range(12):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(w / 40, w / 8)
        img += rng.uniform(-60, 60) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * r * r))
    return np.clip(img + rng.normal(0, 3, img.shape), 0, 255).astype(np.uint8)


def contents(w, h, seed=0):
    rng = np.random.default_rng(seed)
    thermal = (7000 + scene(w, h, seed).astype(np.int64) * 400 // 255).astype(np.uint16)
    thermal.reshape(-1)[rng.choice(thermal.size, 20, replace=False)] = 16383
    return {"thermal": (thermal, 14), "uniform": (rng.integers(0, 65536, (h, w)).astype(np.uint16), 16)}


def modes(bits):
    out = {"equalize": capi.ToneMap.equalize(0, bits)}
    if hasattr(capi.ToneMap, "clahe"):
        out["clahe"] = capi.ToneMap.clahe(8, 8, 0, bits)
        out["clahe-p4"] = capi.ToneMap.clahe(8, 8, 4, bits)
    return out


def med(ts):
    return round(float(np.median(ts)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    nmi.load_library()
    res = {"shape": [W, H], "calls_per_phase": a.iters + a.warmup, "phases": [], "skipped": []}
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    with nmi.NmiContext(W, H) as ctx:
        ctx.set_stream(st.cuda_stream)
        out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
        for f in (1, 4):
            for cname, (px, bits) in contents(f * W, f * H).items():
                src = torch.from_numpy(np.ascontiguousarray(px).view(np.uint8).reshape(-1)).cuda()
                for mname, tm in modes(bits).items():
                    name = f"{f * W}x{f * H}/{cname}/{mname}"
                    try:
                        ctx.set_tone_map(tm)
                    except capi.NmiError:
                        res["skipped"].append(name)     # a library from before CLAHE
                        continue

                    def call():
                        if f == 1:
                            ctx.gray_frame(src, GRAY16, 0, out=out)
                        else:
                            ctx.reduce_frame(src, GRAY16, f, 0, out=out)
                    for _ in range(a.warmup):
                        call()
                    ts = []
                    for _ in range(a.iters):
                        t0 = time.perf_counter()
                        call()
                        ts.append((time.perf_counter() - t0) * 1e6)
                    res["phases"].append({"name": name, "call_us": med(ts), "p10_us": round(float(np.percentile(ts, 10)), 2),
                                          "p90_us": round(float(np.percentile(ts, 90)), 2), "checksum": int(out.sum().item())})
    torch.cuda.set_stream(torch.cuda.default_stream())
    res["phase_names"] = ",".join(p["name"] for p in res["phases"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
