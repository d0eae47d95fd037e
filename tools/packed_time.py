"""Timing of the deep raw formats (nmi_unpack_frame; NMI_FRAME_MONO10P .. BAYER16_*), after tools/valid_time.py.  Prints one JSON line.

Phases, one after the other:
  unpack/<source>/<format>     nmi_unpack_frame of a 2560x1920 source (factor 4 into the 640x480 context) and of a 640x480 one
                               (factor 1), per format: device time per call from a pair of events around `--batch` back-to-back
                               calls, median over `--iters` batches; bytes = the packed rows read + the container written.
  copy/<source>                a device-to-device copy of the container's bytes, timed the same way (bytes: read + written)
  wall/<mode>/<format>         host wall time of nmi_reduce_frame at factor 4, the call ending in a synchronise: MONO12P and GRAY16
                               of the same content, alternated call by call, under SHIFT and EQUALIZE (bits 12)
  pcie/<format>                bytes a stream sends per 2560x1920 frame: computed from nmi_frame_row_bytes, not measured

Kernel times from the profiler: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/packed_time.py --kernels-only
--iters 5, then python tools/summarize_packed_trace.py TRACE.csv (medians per kernel and grid size).
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
FORMATS = {"gray16_be": capi.FRAME_GRAY16_BE, "mono10p": capi.FRAME_MONO10P, "mono12p": capi.FRAME_MONO12P, "raw10": capi.FRAME_RAW10,
           "raw12": capi.FRAME_RAW12, "bayer16_grbg": capi.FRAME_BAYER16_GRBG}


def med(ts):
    return round(float(np.median(ts)), 2)


def mono12p(px):
    """[H,W] 12-bit pixels -> their Mono12p rows (2 pixels in 3 bytes, lsb-packed), flat uint8."""
    p = np.asarray(px, np.int64)
    b = np.zeros((p.shape[0], p.shape[1] // 2 * 3), np.int64)
    b[:, 0::3] = p[:, 0::2] & 255
    b[:, 1::3] = (p[:, 0::2] >> 8) | ((p[:, 1::2] & 15) << 4)
    b[:, 2::3] = p[:, 1::2] >> 4
    return b.astype(np.uint8).reshape(-1)


def device_us(call, batch, iters, stream):
    """Median device time of one call, from events around `batch` calls."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(batch):
        call()
    ts = []
    for _ in range(iters):
        t0.record(stream)
        for _ in range(batch):
            call()
        t1.record(stream)
        t1.synchronize()
        ts.append(t0.elapsed_time(t1) * 1e3 / batch)
    return med(ts)


def kernel_phases(ctx, res, a, stream):
    rng = np.random.default_rng(0)
    for f in (4, 1):
        ws, hs = f * W, f * H
        out = torch.empty((hs, ws), dtype=torch.int16, device="cuda")
        other = torch.empty_like(out)
        for name, fmt in FORMATS.items():
            row = capi.frame_row_bytes(fmt, ws)
            src = torch.from_numpy(rng.integers(0, 256, row * hs, dtype=np.uint8)).cuda()
            us = device_us(lambda: ctx.unpack_frame(src, fmt, f, 0, out=out, sync=False), a.batch, a.iters, stream)
            moved = row * hs + 2 * ws * hs
            res["phases"].append({"name": f"unpack/{ws}x{hs}/{name}", "device_us": us, "bytes": moved, "gb_per_s": round(moved / us / 1e3, 1)})
        us = device_us(lambda: other.copy_(out, non_blocking=True), a.batch, a.iters, stream)
        moved = 4 * ws * hs
        res["phases"].append({"name": f"copy/{ws}x{hs}", "device_us": us, "bytes": moved, "gb_per_s": round(moved / us / 1e3, 1)})


def wall_phases(ctx, res, a):
    f = 4
    px = np.random.default_rng(1).integers(0, 4096, (f * H, f * W)).astype(np.uint16)
    packed = torch.from_numpy(mono12p(px)).cuda()
    dense = torch.from_numpy(px.view(np.uint8).reshape(-1)).cuda()
    out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    for mname, tm in (("shift", capi.ToneMap.shift(12)), ("equalize", capi.ToneMap.equalize(0, 12))):
        ctx.set_tone_map(tm)
        calls = {"mono12p": lambda: ctx.reduce_frame(packed, capi.FRAME_MONO12P, f, 0, out=out),
                 "gray16": lambda: ctx.reduce_frame(dense, capi.FRAME_GRAY16, f, 0, out=out)}
        ts, sums = {k: [] for k in calls}, {}
        for i in range(a.warmup + a.wall_iters):       # the two alternated, call by call
            for k, call in calls.items():
                t0 = time.perf_counter()
                call()
                if i >= a.warmup:
                    ts[k].append((time.perf_counter() - t0) * 1e6)
                sums[k] = int(out.sum().item())
        assert sums["mono12p"] == sums["gray16"]
        for k in calls:
            res["phases"].append({"name": f"wall/{mname}/{k}", "call_us": med(ts[k]), "p10_us": round(float(np.percentile(ts[k], 10)), 2),
                                  "p90_us": round(float(np.percentile(ts[k], 90)), 2), "checksum": sums[k]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50, help="batches per unpack / copy phase")
    ap.add_argument("--batch", type=int, default=20, help="calls between the two events")
    ap.add_argument("--wall-iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true", help="the unpack and copy phases alone (kernel traces)")
    a = ap.parse_args()
    res = {"shape": [W, H], "phases": []}
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    with nmi.NmiContext(W, H) as ctx:
        ctx.set_stream(st.cuda_stream)
        kernel_phases(ctx, res, a, st)
        if not a.kernels_only:
            wall_phases(ctx, res, a)
    torch.cuda.set_stream(torch.cuda.default_stream())
    for name, fmt in {"gray16": capi.FRAME_GRAY16, **FORMATS}.items():   # computed, not measured
        res["phases"].append({"name": f"pcie/{name}", "bytes_per_frame": capi.frame_row_bytes(fmt, 4 * W) * 4 * H})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
