"""Masked search timing: nmi_search_grid against nmi_search_grid_masked on the same 640x480, 27 x 27, 256-bin inputs, once with
all-ones masks and once with the producer's masks of a rotation grid; the per-search count + table build; nmi_warp_stack
against nmi_warp_stack_masked.  Prints one JSON line.

Kernel times come from nmi_set_profiling events (the scoring launches of one call; for the masked search the optimistic
launch and the exact launch after it).  The count + table build is the GPU time of a whole masked call (events on the
context's stream) minus its scoring launches.  Kernel names and per-kernel times: run it under
rocprofv3 --kernel-trace --stats -- python tools/masked_timing.py
Also reports the 729-candidate winner of the rotation grid with and without the border masks.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from orbslam2_nmi_amd import capi, synthetic as sy  # noqa: E402


def kernel_us(ctx, fn, n, warmup):
    ctx.set_profiling(True)
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(n):
        fn()
        ts.append(ctx.last_kernel_ms() * 1000.0)
    ctx.set_profiling(False)
    return float(np.median(ts)), float(np.mean(ts))


def stream_us(stream, fn, n, warmup):
    """GPU time of fn()'s work on `stream` (the context's stream), from torch events around each call."""
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1000.0)
    return float(np.median(ts)), float(np.mean(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    n, warm = args.iters, args.warmup
    w, h, S, Wn = 640, 480, 27, 27
    wl = sy.workload(w, h, S, Wn, seed=1234)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rs, ws = dev(wl["render_stack"]), dev(wl["warp_stack"])
    ones = torch.ones((Wn, h, w), dtype=torch.uint8, device="cuda")
    Ms = sy.warp_homographies(sy.intrinsics(w, h), wl["w_counts"], (0.02, 0.02, 0.05))
    frame = dev(wl["frame"])
    out = {"shape": [w, h], "grid": [Wn, S], "bins": 256, "iters": n, "warmup": warm}
    stream = torch.cuda.Stream()
    with capi.NmiContext(w, h) as ctx:
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            pw, pm = ctx.warp_stack_masked(frame, Ms)  # the rotation grid's warps and their border masks
            ctx.synchronize()
            ratings = torch.zeros((Wn, S), dtype=torch.float32, device="cuda")
            plain = ctx.bind_search(rs, ws)
            out["search_grid_us"] = kernel_us(ctx, plain, n, warm)
            out["search_grid_masked_ones_us"] = kernel_us(ctx, lambda: ctx.search_grid_masked(rs, ws, ones), n, warm)
            out["search_grid_producer_warps_us"] = kernel_us(ctx, lambda: ctx.search_grid(rs, pw), n, warm)
            out["search_grid_masked_producer_us"] = kernel_us(ctx, lambda: ctx.search_grid_masked(rs, pw, pm), n, warm)
            # count + tables = whole masked call on the stream minus its scoring launches (both medians)
            call = stream_us(stream, lambda: ctx.search_grid_masked(rs, pw, pm), n, warm)
            out["masked_call_gpu_us"] = call
            out["count_tables_us_est"] = call[0] - out["search_grid_masked_producer_us"][0]
            wout, mout = torch.empty_like(ws), torch.empty_like(ws)
            out["warp_stack_us"] = stream_us(stream, lambda: ctx.warp_stack(frame, Ms, out=wout, sync=False), n, warm)
            out["warp_stack_masked_us"] = stream_us(stream, lambda: ctx.warp_stack_masked(frame, Ms, out=wout, out_masks=mout, sync=False),
                                                    n, warm)
            # the bias the border masks remove (or not): winner of the rotation grid without and with them
            i0, s0 = ctx.search_grid(rs, pw, ratings)
            i1, s1 = ctx.search_grid_masked(rs, pw, pm, ratings)
            out["winner_unmasked"] = {"index": i0, "warp": i0 // S, "render": i0 % S, "score": float(s0)}
            out["winner_masked"] = {"index": i1, "warp": i1 // S, "render": i1 % S, "score": float(s1)}
            out["planted"] = {"index": int(wl["planted"]), "warp": int(wl["planted"]) // S, "render": int(wl["planted"]) % S}
            out["mask_valid_fraction"] = [round(float(c) / (w * h), 4) for c in ctx.mask_counts(Wn)]
    out["note"] = "(median, mean) in us; kernel times are the scoring launches only (nmi_set_profiling)"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
