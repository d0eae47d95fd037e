"""Depth renders against the colour renders of the same maps (nmi_render_mesh_depth / nmi_render_mesh_colored,
nmi_render_points_depth / nmi_render_points), at the project's own sizes: 27 views at 848x480, the plane at 10 m as 60x40 and
300x200 quads (4,800 and 120,000 triangles) and as a 3 M-point cloud (point size 3).  Prints one JSON line.

Run:      python tools/depth_time.py --iters 300
The two forms of each map are enqueued ALTERNATELY, call by call, on one context; each call is timed by a pair of HIP events
(the whole producer: binning + clip + tiles, or clear + splat + resolve).  The calls are cut into --reps repetitions; per repetition
the median, over the repetitions their median and their spread (min .. max).

Per-kernel times come from the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/depth_time.py --iters 300
    python tools/depth_time.py --trace DIR
The second command reads the kernel trace and prints, per kernel of the tile and resolve families, the same statistic (dispatches in
order, the warm-up share dropped, cut into repetitions): nmi_mesh_tile_kernel<DepthAttr, ...> against
nmi_mesh_tile_kernel<ColoredAttr, ...>, and the resolve kernels with and without a DepthShade.
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

WARM_SHARE = 0.2      # of each kernel's dispatches (and of each form's calls): clocks and caches coming up


def stat(us, reps):
    us = np.asarray(us, float)
    us = us[int(len(us) * WARM_SHARE):]
    per_rep = [float(np.median(c)) for c in np.array_split(us, reps) if len(c)]
    return {"median_of_reps": round(float(np.median(per_rep)), 2), "min_rep": round(min(per_rep), 2), "max_rep": round(max(per_rep), 2),
            "dispatches": int(len(us))}


def read_trace(directory, reps):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    per_kernel = {}
    for f in files:
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                if "mesh_tile" in name or "zbuf_resolve" in name:
                    name = name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").replace("nmi::", "")
                    per_kernel.setdefault(name, []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    # measure() runs the tile kernels on the two meshes in turn, the same number of calls each: the halves of their dispatches
    out = {}
    for name, rows in sorted(per_kernel.items()):
        rows.sort()
        us = [d for _, d in rows]
        if "mesh_tile" in name:
            half = len(us) // 2
            out[name + " (4,800 triangles)"] = stat(us[:half], reps)
            out[name + " (120,000 triangles)"] = stat(us[half:], reps)
        else:
            out[name] = stat(us, reps)
    return out


def bench_mesh(rp, w, h, nx, ny):
    """bench.py run_e2e_config's mesh (tools/mesh_color_time.py): positions only -> xyz [3T,3]."""
    uu, vv = np.meshgrid(np.linspace(-w, 2 * w, nx + 1), np.linspace(-h, 2 * h, ny + 1))
    P = np.stack([(uu - rp.cx) / rp.fx * 10.0, (vv - rp.cy) / rp.fy * 10.0, np.full_like(uu, 10.0)], -1).astype(np.float32)
    p00, p10, p01, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    return np.ascontiguousarray(np.stack([p00, p11, p10, p00, p01, p11], 2).reshape(-1, 3))


def bench_cloud(rp, w, h):
    """tools/color_time.py level_scene's cloud: the same plane as ~3 M points."""
    nu, nv = int(3 * w * 0.9), int(3 * h * 0.9)
    uu, vv = np.meshgrid(np.linspace(-w, 2 * w, nu), np.linspace(-h, 2 * h, nv))
    return np.stack([(uu - rp.cx) / rp.fx * 10.0, (vv - rp.cy) / rp.fy * 10.0, np.full_like(uu, 10.0)], -1).reshape(-1, 3).astype(np.float32)


def alternate(torch, st, forms, iters, warmup, reps):
    """forms: {name: callable that enqueues one render} -> {name: stat of the per-call event times}."""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in forms}
    for i in range(iters):
        for k, fn in forms.items():
            e0, e1 = ev[k][i]
            e0.record(st)
            fn()
            e1.record(st)
    torch.cuda.synchronize()
    return {k: stat([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[k]], reps) for k in forms}


def measure(iters, warmup, reps):
    import torch
    import orbslam2_nmi_amd as nmi
    from orbslam2_nmi_amd import capi, hostapi as H, synthetic as sy
    w, h = 848, 480
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=5.0, far_plane=30.0, point_size=3.0)
    shade = capi.NmiDepthShade(near_plane=5.0, far_plane=30.0, scale=1000.0, lo=5000, hi=20000)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    out = {"shape": [w, h], "views": 27, "iters": iters, "warmup": warmup, "reps": reps,
           "note": "us per call, HIP events around each producer call, the forms of a map alternating; per repetition the median"}
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_stream(st.cuda_stream)
        Twc = np.eye(4, dtype=np.float32)
        pos, look, up = Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]
        g = H.SearchKernel.make([3] * 6, [0.2, 0.2, 0.5, 0.02, 0.02, 0.05])
        cells = [(sx, sy_, sz) for sz in range(3) for sy_ in range(3) for sx in range(3)]
        mvps = np.stack([capi.render_mvp(rp, pos, look, up, H.calculate_translation(Twc, g, *c)) for c in cells])
        S = len(mvps)
        grey = torch.empty((S, h, w), dtype=torch.uint8, device="cuda")
        grey2 = torch.empty_like(grey)
        mask = torch.empty_like(grey)
        d16 = torch.empty((S, h, w), dtype=torch.int16, device="cuda")
        for nx, ny in ((60, 40), (300, 200)):
            xyz = bench_mesh(rp, w, h, nx, ny)
            dx = torch.from_numpy(xyz).cuda()
            red = torch.from_numpy(np.random.default_rng(7).uniform(0, 1, len(xyz)).astype(np.float32)).cuda()
            if float((ctx.render_mesh_colored(dx, red, mvps[13:14])[0] != 255).float().mean()) < 0.9:   # back faces are culled: turn the triangles round
                flip = torch.tensor([0, 2, 1], device="cuda")
                dx = dx.view(-1, 3, 3)[:, flip].reshape(-1, 3).contiguous()
            cov = float((ctx.render_mesh_depth(dx, mvps[13:14], shade, out_masks=True)[1] != 0).float().mean())
            forms = {"colored": lambda: ctx.render_mesh_colored(dx, red, mvps, out=grey, sync=False),
                     "depth": lambda: ctx.render_mesh_depth(dx, mvps, shade, out=grey2, sync=False),
                     "colored_masked": lambda: ctx.render_mesh_colored_masked(dx, red, mvps, out=grey, out_masks=mask, sync=False),
                     "depth_masked_depth16": lambda: ctx.render_mesh_depth(dx, mvps, shade, out=grey2, out_masks=mask, depth16=d16, sync=False)}
            res = alternate(torch, st, forms, iters, warmup, reps)
            res["triangles"] = int(len(xyz) // 3)
            res["covered_share_of_the_centre_view"] = round(cov, 3)
            out[f"mesh_{nx}x{ny}"] = res
            ctx.synchronize()
        xyz = bench_cloud(rp, w, h)
        dx = torch.from_numpy(xyz).cuda()
        red = torch.from_numpy(np.random.default_rng(8).uniform(0, 1, len(xyz)).astype(np.float32)).cuda()
        forms = {"colour": lambda: ctx.render_points(dx, red, mvps, 3.0, out=grey, sync=False),
                 "depth": lambda: ctx.render_points_depth(dx, red, mvps, 3.0, shade, out=grey2, sync=False),
                 "colour_masked": lambda: ctx.render_points_masked(dx, red, mvps, 3.0, out=grey, out_masks=mask, sync=False),
                 "depth_masked_depth16": lambda: ctx.render_points_depth(dx, red, mvps, 3.0, shade, out=grey2, out_masks=mask, depth16=d16, sync=False)}
        res = alternate(torch, st, forms, iters, warmup, reps)
        res["points"] = int(len(xyz))
        out["cloud"] = res
        ctx.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300, help="timed calls of each form")
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", help="read a rocprofv3 --kernel-trace output directory instead of measuring")
    a = ap.parse_args()
    print(json.dumps(read_trace(a.trace, a.reps) if a.trace else measure(a.iters, a.warmup, a.reps)))


if __name__ == "__main__":
    main()
