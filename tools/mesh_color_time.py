"""Coloured mesh level against the textured mesh level, on the two meshes and the views of bench.py --config e2e --map mesh
(the plane at 10 m as 60x40 and 300x200 quads = 4,800 and 120,000 triangles, 848x480, 27 views x 27 warps, the three grid levels'
parameter sets in turn).  The colours are the texture's luma sampled at the corners.  Prints one JSON line.

Both levels live on one context and are replayed ALTERNATELY, replay by replay, after a warm-up that brings the clocks up; each
replay is timed by a pair of HIP events on the context's stream around nmi_level_run (graph launch -> the search's last kernel).
The replays are cut into --reps repetitions; per repetition the median, over the repetitions their median and their spread
(min .. max): the spread of the textured level is the yardstick for "not slower".

Per-kernel times: run it under  rocprofv3 --kernel-trace --stats -- python tools/mesh_color_time.py --iters 300
(the coloured tile kernels carry _color in their names; the passes in front of them are the textured mesh's).
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
from orbslam2_nmi_amd import capi, hostapi as H, synthetic as sy  # noqa: E402


def bench_mesh(rp, w, h, nx, ny, B):
    """bench.py run_e2e_config's mesh: -> xyz [3T,3], uv [3T,2], and the texture's luma at the corners [3T] (nearest texel)."""
    uu, vv = np.meshgrid(np.linspace(-w, 2 * w, nx + 1), np.linspace(-h, 2 * h, ny + 1))
    P = np.stack([(uu - rp.cx) / rp.fx * 10.0, (vv - rp.cy) / rp.fy * 10.0, np.full_like(uu, 10.0)], -1).astype(np.float32)
    T = np.stack([(uu + w) / (3 * w), (vv + h) / (3 * h)], -1).astype(np.float32)
    p00, p10, p01, p11 = P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]
    t00, t10, t01, t11 = T[:-1, :-1], T[:-1, 1:], T[1:, :-1], T[1:, 1:]
    xyz = np.ascontiguousarray(np.stack([p00, p11, p10, p00, p01, p11], 2).reshape(-1, 3))
    uv = np.ascontiguousarray(np.stack([t00, t11, t10, t00, t01, t11], 2).reshape(-1, 2))
    th, tw = B.shape
    ti = np.clip((uv[:, 0] * tw).astype(int), 0, tw - 1)
    tj = np.clip((uv[:, 1] * th).astype(int), 0, th - 1)
    red = np.ascontiguousarray(B[tj, ti].astype(np.float32) / np.float32(255))
    return xyz, uv, red


def one_mesh(nx, ny, iters, warmup, reps):
    w, h, levels = 848, 480, 3
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=5.0, far_plane=30.0, point_size=3.0)
    B = sy.scene(2 * w, 2 * h, 77)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    xyz, uv, red = bench_mesh(rp, w, h, nx, ny, B)
    out = {"quads": [nx, ny], "triangles": int(xyz.shape[0] // 3), "shape": [w, h], "grid": [27, 27], "iters": iters, "warmup": warmup, "reps": reps}
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_stream(st.cuda_stream)
        tex = nmi.NmiTexture(ctx, np.stack([B, B, B], -1).astype(np.uint8))
        dx, du, dc = torch.from_numpy(xyz).cuda(), torch.from_numpy(uv).cuda(), torch.from_numpy(red).cuda()
        Twc = np.eye(4, dtype=np.float32)
        pos, look, up = Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]
        grids = [H.SearchKernel.make([3] * 6, [s / 2 ** l for s in (0.2, 0.2, 0.5, 0.02, 0.02, 0.05)]) for l in range(levels)]
        cells = [(sx, sy_, sz) for sz in range(3) for sy_ in range(3) for sx in range(3)]
        mvps = [np.stack([capi.render_mvp(rp, pos, look, up, H.calculate_translation(Twc, g, *c)) for c in cells]) for g in grids]
        homs = [capi.warp_homographies(K, (3, 3, 3), tuple(g.step[3:6])) for g in grids]
        centre = capi.render_mvp(rp, pos, look, up, (0, 0, 0))[None]
        frame = ctx.render_mesh(dx, du, tex, centre)[0]
        if float((frame != 255).float().mean()) < 0.9:  # back faces are culled: turn every triangle round, as bench.py does
            flip = torch.tensor([0, 2, 1], device="cuda")
            dx = dx.view(-1, 3, 3)[:, flip].reshape(-1, 3).contiguous()
            du = du.view(-1, 3, 2)[:, flip].reshape(-1, 2).contiguous()
            dc = dc.view(-1, 3)[:, flip].reshape(-1).contiguous()
            frame = ctx.render_mesh(dx, du, tex, centre)[0]
        assert float((frame != 255).float().mean()) >= 0.9, "the mesh does not cover the view"
        lut = torch.clamp(torch.round(255.0 * (torch.arange(256, device="cuda") / 255.0) ** 0.5), 0, 255).to(torch.uint8)
        frame = lut[torch.flip(frame, dims=[0]).long()].contiguous()
        noise = torch.from_numpy(np.random.default_rng(4242).normal(0.0, 10.0, (h, w)).astype(np.float32)).cuda()
        frame = torch.clamp(torch.round(frame.float() + noise), 0, 255).to(torch.uint8).contiguous()
        # how far the coloured render is from the textured one (the colours are the texture at the corners, no more)
        a = ctx.render_mesh(dx, du, tex, centre)[0].float()
        b = ctx.render_mesh_colored(dx, dc, centre)[0].float()
        out["mean_abs_grey_difference_colored_vs_textured"] = round(float((a - b).abs().mean()), 2)
        torch.cuda.synchronize()
        lv = {"textured": nmi.NmiLevel(ctx, dx, du, frame, 27, 27, 3.0, texture=tex),
              "colored": nmi.NmiLevel(ctx, dx, dc, frame, 27, 27, 3.0, colors=True)}
        runs = {k: [v.bind(mvps[l], homs[l]) for l in range(levels)] for k, v in lv.items()}
        res = {}
        for i in range(warmup):
            for k in runs:
                res[k] = runs[k][i % levels]()
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in runs}
        for i in range(iters):
            for k in runs:
                e0, e1 = ev[k][i]
                e0.record(st)
                res[k] = runs[k][i % levels]()
                e1.record(st)
        torch.cuda.synchronize()
        for k in runs:
            us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[k]])
            per_rep = [float(np.median(c)) for c in np.array_split(us, reps)]
            out[k + "_level_us"] = {"median_of_reps": round(float(np.median(per_rep)), 2), "min_rep": round(min(per_rep), 2),
                                    "max_rep": round(max(per_rep), 2), "reps": [round(v, 2) for v in per_rep]}
            out["winner_" + k] = [int(res[k][0]), float(res[k][1])]
        t, c = out["textured_level_us"], out["colored_level_us"]
        out["colored_over_textured"] = round(c["median_of_reps"] / t["median_of_reps"], 4)
        out["colored_not_slower_beyond_textured_spread"] = bool(c["median_of_reps"] <= t["median_of_reps"] + (t["max_rep"] - t["min_rep"]))
        for v in lv.values():
            v.close()
        tex.close()
    torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1500, help="timed replays of each level (a multiple of --reps x 3)")
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 5, "at least five repetitions"
    out = {"mesh_60x40": one_mesh(60, 40, args.iters, args.warmup, args.reps), "mesh_300x200": one_mesh(300, 200, args.iters, args.warmup, args.reps),
           "note": "us per level replay, HIP events around nmi_level_run, textured and coloured replays alternating; per repetition the median"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
