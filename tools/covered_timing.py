"""Covered search timing: nmi_search_grid, nmi_search_grid_masked and nmi_search_grid_covered on the same 640x480, 27 x 27,
256-bin inputs -- all-ones masks, then the producer's border masks of a rotation grid with the coverage of a real point-cloud
render -- and each nmi_render_*_masked call against its unmasked form.  Prints one JSON line.

Search times come from nmi_set_profiling events (the scoring launches of one call: for the masked and covered searches the
optimistic launch and the exact launch after it; the masked search's count + table build before them is not included, the
covered search has none).  Render times are the GPU time of a whole call on the context's stream.  Kernel names and
per-kernel times: run it under  rocprofv3 --kernel-trace --stats -- python tools/covered_timing.py
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

import orbslam2_nmi_amd as nmi  # noqa: E402
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
    ones_w = torch.ones((Wn, h, w), dtype=torch.uint8, device="cuda")
    ones_r = torch.ones((S, h, w), dtype=torch.uint8, device="cuda")
    K = sy.intrinsics(w, h)
    Ms = sy.warp_homographies(K, wl["w_counts"], (0.02, 0.02, 0.05))
    frame = dev(wl["frame"])
    # a point cloud that covers part of the view: its renders' coverage is the map-side mask
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=0.5, far_plane=40.0, point_size=3.0)
    rng = np.random.default_rng(1)
    npts = 200000
    xyz = np.stack([rng.uniform(-6, 2, npts), rng.uniform(-3, 3, npts), rng.uniform(8, 12, npts)], -1).astype(np.float32)
    red = rng.uniform(0, 1, npts).astype(np.float32)
    mvps = np.stack([capi.render_mvp(rp, (0, 0, 0), (0, 0, 1), (0, -1, 0), tuple(rng.uniform(-0.3, 0.3, 3))) for _ in range(S)])
    dx, dr = dev(xyz), dev(red)
    # a mesh for the mesh renderer's pair: a relief over part of the view
    us, vs = np.linspace(0.1 * w, 0.7 * w, 61), np.linspace(0.1 * h, 0.9 * h, 41)
    uu, vv = np.meshgrid(us, vs)
    z = 10.0 + np.sin(uu * 0.02)
    P = np.stack([(uu - rp.cx) / rp.fx * z, (vv - rp.cy) / rp.fy * z, z], -1).astype(np.float32)
    T = np.stack([uu / w, vv / h], -1).astype(np.float32)
    p00, p10, p01, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    t00, t10, t01, t11 = T[:-1, :-1], T[:-1, 1:], T[1:, :-1], T[1:, 1:]
    mx = np.concatenate([np.stack([p00, p10, p11, p00, p11, p01], 2).reshape(-1, 3), np.stack([p00, p11, p10, p00, p01, p11], 2).reshape(-1, 3)])
    mu = np.concatenate([np.stack([t00, t10, t11, t00, t11, t01], 2).reshape(-1, 2), np.stack([t00, t11, t10, t00, t01, t11], 2).reshape(-1, 2)])
    dmx, dmu = dev(mx), dev(mu)
    rgb = np.stack([sy.scene(256, 256, 5)] * 3, -1).astype(np.uint8)
    out = {"shape": [w, h], "grid": [Wn, S], "bins": 256, "iters": n, "warmup": warm}
    stream = torch.cuda.Stream()
    with capi.NmiContext(w, h) as ctx, nmi.NmiTexture(ctx, rgb) as tex:
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            pw, pm = ctx.warp_stack_masked(frame, Ms)  # the rotation grid's warps and their border masks
            prs, prm = ctx.render_points_masked(dx, dr, mvps, 3.0)  # renders of the cloud and their coverage
            ctx.synchronize()
            plain = ctx.bind_search(rs, ws)
            out["search_grid_us"] = kernel_us(ctx, plain, n, warm)
            out["search_grid_masked_ones_us"] = kernel_us(ctx, lambda: ctx.search_grid_masked(rs, ws, ones_w), n, warm)
            out["search_grid_covered_ones_us"] = kernel_us(ctx, lambda: ctx.search_grid_covered(rs, ones_r, ws, ones_w), n, warm)
            out["search_grid_cloud_renders_us"] = kernel_us(ctx, lambda: ctx.search_grid(prs, pw), n, warm)
            out["search_grid_covered_border_coverage_us"] = kernel_us(ctx, lambda: ctx.search_grid_covered(prs, prm, pw, pm), n, warm)
            out["covered_call_gpu_us"] = stream_us(stream, lambda: ctx.search_grid_covered(prs, prm, pw, pm), n, warm)
            counts = ctx.cover_counts(Wn * S)
            out["cover_fraction_min_max"] = [round(float(counts.min()) / (w * h), 4), round(float(counts.max()) / (w * h), 4)]
            ro, mo_ = torch.empty_like(prs), torch.empty_like(prm)
            out["render_points_us"] = stream_us(stream, lambda: ctx.render_points(dx, dr, mvps, 3.0, out=ro, sync=False), n, warm)
            out["render_points_masked_us"] = stream_us(stream, lambda: ctx.render_points_masked(dx, dr, mvps, 3.0, out=ro, out_masks=mo_, sync=False),
                                                       n, warm)
            out["render_mesh_us"] = stream_us(stream, lambda: ctx.render_mesh(dmx, dmu, tex, mvps, out=ro, sync=False), n, warm)
            out["render_mesh_masked_us"] = stream_us(stream, lambda: ctx.render_mesh_masked(dmx, dmu, tex, mvps, out=ro, out_masks=mo_, sync=False),
                                                     n, warm)
    out["note"] = "(median, mean) in us; search times are the scoring launches only (nmi_set_profiling)"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
