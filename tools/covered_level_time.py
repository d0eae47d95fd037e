"""Covered level timing (nmi_level_set_coverage) and covered mid-size search timing (nmi_covered_pix_kernel).  Prints one JSON line.

1. Captured level, 27 x 27 at 848x480, on three maps: the point cloud of tools/level_time.py (2.97 M points), the textured mesh
   of examples/level_pipeline --mesh 60x40 (its surface and texture function, 4,800 triangles spanning three frame widths:
   every pixel of every render is covered), and a partial-coverage relief (4,800 triangles over part of the view, 48 % of each
   render covered; the rest keeps the clear colour 255, whose few bins wrap 16-bit counters, so the unmasked and masked
   searches redo candidates exactly).  Per map an unmasked level, a masked one (border masks of the rotation warps + a hood
   over the bottom sixth of the frame) and a covered one (coverage + border masks + the same hood), replayed ALTERNATELY in the
   same loop, host wall time of each nmi_level_run (parameters in -> winner out), the same parameters every replay.
2. Covered 81- and 108-candidate searches at 640x480 with the border masks of a rotation grid and the coverage of a point
   cloud's renders: default routing (pixel ranges) against NMI_OPT_SPLIT 0 (nmi_covered_grid_kernel) and against the unmasked
   search on the same stacks (nmi_pix_kernel), the three alternated call by call, scoring launches timed by nmi_set_profiling.

Per-kernel times: run it under rocprofv3 --kernel-trace --stats -- python tools/covered_level_time.py --iters 200
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbslam2_nmi_amd as nmi  # noqa: E402
from orbslam2_nmi_amd import capi, hostapi as H, synthetic as sy  # noqa: E402


def med(ts):
    return float(np.median(ts)), float(np.mean(ts))


def surface_mesh(rp, w, h, nx=60, ny=40, seed=7):
    """examples/level_pipeline.cpp --mesh NXxNY: the surface z = 10 + 3 sin(0.012 u) cos(0.015 v) over u in [-W, 2W], v in
    [-H, 2H] as nx x ny quads (two triangles each, that program's winding), and its texture function on a 2048 x 1024 raster
    (the texture noise from numpy rather than that program's generator).  -> (xyz [3T,3], uv [3T,2], rgb [1024,2048,3])"""
    i, j = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    u, v = (-w + 3.0 * w * i / nx).astype(np.float32), (-h + 3.0 * h * j / ny).astype(np.float32)
    z = (10.0 + 3.0 * np.sin(0.012 * u) * np.cos(0.015 * v)).astype(np.float32)
    P = np.stack([(u - rp.cx) / rp.fx * z, (v - rp.cy) / rp.fy * z, z], -1).astype(np.float32)
    T = np.stack([i / nx, j / ny], -1).astype(np.float32)
    p00, p10, p01, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    t00, t10, t01, t11 = T[:-1, :-1], T[:-1, 1:], T[1:, :-1], T[1:, 1:]
    xyz = np.stack([p00, p11, p10, p00, p01, p11], 2).reshape(-1, 3)
    uv = np.stack([t00, t11, t10, t00, t01, t11], 2).reshape(-1, 2)
    tw, th = 2048, 1024
    ti, tj = np.meshgrid(np.arange(tw), np.arange(th))
    tu, tv = -w + 3.0 * w * (ti + 0.5) / tw, -h + 3.0 * h * (tj + 0.5) / th
    n = np.random.default_rng(seed).uniform(-0.5, 0.5, (th, tw))
    g = (128.0 + 45.0 * np.sin(0.031 * tu + 0.6 * np.sin(0.017 * tv)) + 40.0 * np.cos(0.043 * tv + 0.011 * tu) + 18.0 * np.sin(0.11 * (tu + tv))
         + 10.0 * n)
    g = np.rint(np.clip(g, 0, 255)).astype(np.uint8)
    return xyz, uv, np.stack([g] * 3, -1)


def relief_mesh(rp, w, h, nx=40, ny=30):
    """nx x ny quads of a relief over part of the view, both windings: 4 nx ny triangles."""
    us, vs = np.linspace(0.1 * w, 0.7 * w, nx + 1), np.linspace(0.1 * h, 0.9 * h, ny + 1)
    uu, vv = np.meshgrid(us, vs)
    z = 10.0 + np.sin(uu * 0.02)
    P = np.stack([(uu - rp.cx) / rp.fx * z, (vv - rp.cy) / rp.fy * z, z], -1).astype(np.float32)
    T = np.stack([uu / w, vv / h], -1).astype(np.float32)
    p00, p10, p01, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    t00, t10, t01, t11 = T[:-1, :-1], T[:-1, 1:], T[1:, :-1], T[1:, 1:]
    mx = np.concatenate([np.stack([p00, p10, p11, p00, p11, p01], 2).reshape(-1, 3), np.stack([p00, p11, p10, p00, p01, p11], 2).reshape(-1, 3)])
    mu = np.concatenate([np.stack([t00, t10, t11, t00, t11, t01], 2).reshape(-1, 2), np.stack([t00, t11, t10, t00, t01, t11], 2).reshape(-1, 2)])
    return mx, mu


def level_part(iters, warmup, scene):
    w, h = 848, 480
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=5.0, far_plane=30.0, point_size=3.0)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    out = {"shape": [w, h], "grid": [27, 27], "iters": iters, "warmup": warmup, "map": scene}
    mesh = scene != "cloud"
    if mesh:
        if scene == "surface":
            mx, mu, rgb = surface_mesh(rp, w, h)
        else:
            mx, mu = relief_mesh(rp, w, h)
            rgb = np.stack([sy.scene(256, 256, 5)] * 3, -1).astype(np.uint8)
        dx, da = torch.from_numpy(mx).cuda(), torch.from_numpy(mu).cuda()
        out["triangles"] = int(mx.shape[0] // 3)
    else:
        # tools/level_time.py's cloud
        B = sy.scene(2 * w, 2 * h, 77)
        nu, nv = int(3 * w * 0.9), int(3 * h * 0.9)
        uu, vv = np.meshgrid(np.linspace(-w, 2 * w, nu), np.linspace(-h, 2 * h, nv))
        xyz = np.stack([(uu - rp.cx) / rp.fx * 10.0, (vv - rp.cy) / rp.fy * 10.0, np.full_like(uu, 10.0)], -1).reshape(-1, 3).astype(np.float32)
        red = (B[np.clip(((vv + h) / 3 * 2).astype(int), 0, 2 * h - 1), np.clip(((uu + w) / 3 * 2).astype(int), 0, 2 * w - 1)].astype(np.float32)
               / np.float32(256)).reshape(-1)
        dx, da = torch.from_numpy(xyz).cuda(), torch.from_numpy(red).cuda()
        out["points"] = int(xyz.shape[0])
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_stream(st.cuda_stream)
        tex = nmi.NmiTexture(ctx, rgb) if mesh else None
        Twc = np.eye(4, dtype=np.float32)
        if scene != "surface":
            Twc[:3, 1] = [0, -1, 0]  # (examples/level_pipeline's pose is the identity: its triangles face that camera)
        pos, look, up = Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]
        g = H.SearchKernel.make([3] * 6, [0.2, 0.2, 0.5, 0.02, 0.02, 0.05])
        cells = [(sx, sy_, sz) for sz in range(3) for sy_ in range(3) for sx in range(3)]
        mvps = np.stack([capi.render_mvp(rp, pos, look, up, H.calculate_translation(Twc, g, *c)) for c in cells])
        homs = capi.warp_homographies(K, (3, 3, 3), tuple(g.step[3:6]))
        v0 = capi.render_mvp(rp, pos, look, up, (0, 0, 0))[None]
        fr = ctx.render_mesh(dx, da, tex, v0)[0] if mesh else ctx.render_points(dx, torch.sqrt(da), v0, 3.0)[0]
        frame = torch.flip(fr, dims=[0]).contiguous()
        hood = torch.ones((h, w), dtype=torch.uint8, device="cuda")
        hood[h - h // 6:] = 0
        torch.cuda.synchronize()
        levels = {k: nmi.NmiLevel(ctx, dx, da, frame, 27, 27, 3.0, texture=tex) for k in ("unmasked", "masked", "covered")}
        levels["masked"].set_masks(True, hood)
        levels["covered"].set_coverage(True, hood)
        runs = {k: lv.bind(mvps, homs) for k, lv in levels.items()}
        for _ in range(warmup):
            for r in runs.values():
                r()
        ts = {k: [] for k in runs}
        res = {}
        for _ in range(iters):
            for k, r in runs.items():
                t0 = time.perf_counter()
                res[k] = r()
                ts[k].append((time.perf_counter() - t0) * 1e6)
        for k in runs:
            out[k + "_level_us"] = med(ts[k])
            out["winner_" + k] = [int(res[k][0]), float(res[k][1])]
        out["masked_over_unmasked"] = out["masked_level_us"][0] / out["unmasked_level_us"][0]
        out["covered_over_unmasked"] = out["covered_level_us"][0] / out["unmasked_level_us"][0]
        out["covered_over_masked"] = out["covered_level_us"][0] / out["masked_level_us"][0]
        rm, wm, cnt = levels["covered"].coverage()
        out["render_covered_fraction"] = round(float(np.count_nonzero(rm)) / rm.size, 4)
        out["len_fraction_min_max"] = [round(float(cnt.min()) / (w * h), 4), round(float(cnt.max()) / (w * h), 4)]
        for lv in levels.values():
            lv.close()
        if tex is not None:
            tex.close()
    torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def search_part(iters, warmup, S, Wn):
    w, h = 640, 480
    wl = sy.workload(w, h, S, Wn, seed=99)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rs, frame = dev(wl["render_stack"]), dev(wl["frame"])
    Ms = sy.warp_homographies(sy.intrinsics(w, h), wl["w_counts"], (0.02, 0.02, 0.05))
    # the coverage of a sparse point cloud's renders (tools/covered_timing.py's cloud)
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=5.0, far_plane=30.0, point_size=3.0)
    rng = np.random.default_rng(1)
    npts = 200000
    xyz = np.stack([rng.uniform(-6, 2, npts), rng.uniform(-3, 3, npts), rng.uniform(8, 12, npts)], -1).astype(np.float32)
    mvps = np.stack([capi.render_mvp(rp, (0, 0, 0), (0, 0, 1), (0, -1, 0), tuple(rng.uniform(-0.3, 0.3, 3))) for _ in range(S)])
    out = {"shape": [w, h], "grid": [Wn, S], "iters": iters, "warmup": warmup}
    stream = torch.cuda.Stream()
    ctxs = [capi.NmiContext(w, h) for _ in range(3)]
    try:
        for c in ctxs:
            c.set_stream(stream.cuda_stream)
        ctxs[1].set_option(ctxs[1].OPT_SPLIT, 0)
        with torch.cuda.stream(stream):
            ws, wm = ctxs[0].warp_stack_masked(frame, Ms)
            _, rm = ctxs[0].render_points_masked(dev(xyz), dev(rng.uniform(0, 1, npts).astype(np.float32)), mvps, 3.0)
            ctxs[0].synchronize()
            calls = {
                "covered_pixel_ranges": (ctxs[0], lambda: ctxs[0].search_grid_covered(rs, rm, ws, wm)),
                "covered_grid_kernel": (ctxs[1], lambda: ctxs[1].search_grid_covered(rs, rm, ws, wm)),
                "unmasked_pixel_ranges": (ctxs[2], lambda: ctxs[2].search_grid(rs, ws)),
            }
            res = {k: None for k in calls}
            for c, _ in calls.values():
                c.set_profiling(True)
            for _ in range(warmup):
                for k, (c, fn) in calls.items():
                    res[k] = fn()
            ts = {k: [] for k in calls}
            for _ in range(iters):
                for k, (c, fn) in calls.items():
                    fn()
                    ts[k].append(c.last_kernel_ms() * 1000.0)
            for k, (c, _) in calls.items():
                c.set_profiling(False)
                out[k + "_us"] = med(ts[k])
                out[k + "_ranges"] = c.pix_status()["last_launch_ranges"]
            assert res["covered_pixel_ranges"] == res["covered_grid_kernel"], res
            out["covered_ranges_over_grid"] = out["covered_pixel_ranges_us"][0] / out["covered_grid_kernel_us"][0]
            out["covered_ranges_over_unmasked_ranges"] = out["covered_pixel_ranges_us"][0] / out["unmasked_pixel_ranges_us"][0]
            out["healed"] = ctxs[0].pix_status()["healed"]
            cnt = ctxs[0].cover_counts(S * Wn)
            out["len_fraction_min_max"] = [round(float(cnt.min()) / (w * h), 4), round(float(cnt.max()) / (w * h), 4)]
    finally:
        for c in ctxs:
            c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    out = {"level_cloud": level_part(args.iters, args.warmup, "cloud"), "level_mesh": level_part(args.iters, args.warmup, "surface"),
           "level_mesh_partial_coverage": level_part(args.iters, args.warmup, "relief"),
           "search81": search_part(args.iters, args.warmup, 9, 9), "search108": search_part(args.iters, args.warmup, 12, 9),
           "note": "(median, mean) in us; level: host wall time of nmi_level_run; search: scoring launches (nmi_set_profiling)"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
