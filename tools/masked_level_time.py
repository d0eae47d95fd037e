"""Masked level timing (nmi_level_set_masks) and masked mid-size search timing (nmi_masked_pix_kernel).  Prints one JSON line.

1. Captured level, 27 x 27 at 848x480 on tools/level_time.py's cloud: an unmasked level and a masked one (border masks of
   the rotation warps + a hood over the bottom sixth of the frame), replayed ALTERNATELY in the same loop, host wall time of
   each nmi_level_run (parameters in -> winner out).  Steady state: the same view and warp parameters every replay (the
   strategy's level; the counts repeat, so no table is rebuilt).  "After a change": the masked level alternates between two
   warp sets, so every replay rebuilds all tables (the first replay of a new strategy level).
2. Masked 81-candidate search (9 renders x 9 warps) at 640x480 with the border masks of a rotation grid: default routing
   (pixel ranges) against NMI_OPT_SPLIT 0 (nmi_masked_grid_kernel) and against the unmasked search (nmi_pix_kernel), the
   three alternated call by call, scoring launches timed by nmi_set_profiling events.

Per-kernel times: run it under rocprofv3 --kernel-trace --stats -- python tools/masked_level_time.py --iters 200
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


def level_part(iters, warmup):
    # tools/level_time.py's cloud and strategy level
    w, h = 848, 480
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=5.0, far_plane=30.0, point_size=3.0)
    B = sy.scene(2 * w, 2 * h, 77)
    nu, nv = int(3 * w * 0.9), int(3 * h * 0.9)
    uu, vv = np.meshgrid(np.linspace(-w, 2 * w, nu), np.linspace(-h, 2 * h, nv))
    xyz = np.stack([(uu - rp.cx) / rp.fx * 10.0, (vv - rp.cy) / rp.fy * 10.0, np.full_like(uu, 10.0)], -1).reshape(-1, 3).astype(np.float32)
    red = (B[np.clip(((vv + h) / 3 * 2).astype(int), 0, 2 * h - 1), np.clip(((uu + w) / 3 * 2).astype(int), 0, 2 * w - 1)].astype(np.float32)
           / np.float32(256)).reshape(-1)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    dx, dr = torch.from_numpy(xyz).cuda(), torch.from_numpy(red).cuda()
    out = {"shape": [w, h], "grid": [27, 27], "points": int(xyz.shape[0]), "iters": iters, "warmup": warmup}
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_stream(st.cuda_stream)
        Twc = np.eye(4, dtype=np.float32)
        Twc[:3, 1] = [0, -1, 0]
        pos, look, up = Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]
        g = H.SearchKernel.make([3] * 6, [0.2, 0.2, 0.5, 0.02, 0.02, 0.05])
        cells = [(sx, sy_, sz) for sz in range(3) for sy_ in range(3) for sx in range(3)]
        mvps = np.stack([capi.render_mvp(rp, pos, look, up, H.calculate_translation(Twc, g, *c)) for c in cells])
        homs = capi.warp_homographies(K, (3, 3, 3), tuple(g.step[3:6]))
        homs2 = capi.warp_homographies(K, (3, 3, 3), tuple(0.5 * np.asarray(g.step[3:6])))
        frame = torch.flip(ctx.render_points(dx, torch.sqrt(dr), capi.render_mvp(rp, pos, look, up, (0, 0, 0))[None], 3.0)[0], dims=[0]).contiguous()
        hood = torch.ones((h, w), dtype=torch.uint8, device="cuda")
        hood[h - h // 6:] = 0
        torch.cuda.synchronize()
        plain = nmi.NmiLevel(ctx, dx, dr, frame, 27, 27, 3.0)
        masked = nmi.NmiLevel(ctx, dx, dr, frame, 27, 27, 3.0)
        masked.set_masks(True, hood)
        run_p, run_m = plain.bind(mvps, homs), masked.bind(mvps, homs)
        run_m2 = masked.bind(mvps, homs2)
        for _ in range(warmup):
            run_p(), run_m()
        tp, tm = [], []
        for _ in range(iters):
            t0 = time.perf_counter()
            rp_ = run_p()
            t1 = time.perf_counter()
            rm_ = run_m()
            t2 = time.perf_counter()
            tp.append((t1 - t0) * 1e6)
            tm.append((t2 - t1) * 1e6)
        out["unmasked_level_us"] = med(tp)
        out["masked_level_us"] = med(tm)
        out["masked_over_unmasked"] = out["masked_level_us"][0] / out["unmasked_level_us"][0]
        out["winner_unmasked"], out["winner_masked"] = [int(rp_[0]), float(rp_[1])], [int(rm_[0]), float(rm_[1])]
        # every replay after a change of warps: all 27 tables rebuilt
        tc, tu = [], []
        for i in range(max(iters // 5, 50)):
            t0 = time.perf_counter()
            run_m2() if i % 2 == 0 else run_m()
            t1 = time.perf_counter()
            run_p()
            t2 = time.perf_counter()
            tc.append((t1 - t0) * 1e6)
            tu.append((t2 - t1) * 1e6)
        out["masked_level_after_warp_change_us"] = med(tc)
        out["unmasked_level_same_loop_us"] = med(tu)
        counts = masked.masks()[1]
        out["mask_valid_fraction"] = [round(float(c) / (w * h), 4) for c in counts]
        plain.close()
        masked.close()
    torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def search_part(iters, warmup):
    w, h, S, Wn = 640, 480, 9, 9
    wl = sy.workload(w, h, S, Wn, seed=99)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rs, frame = dev(wl["render_stack"]), dev(wl["frame"])
    Ms = sy.warp_homographies(sy.intrinsics(w, h), wl["w_counts"], (0.02, 0.02, 0.05))
    out = {"shape": [w, h], "grid": [Wn, S], "iters": iters, "warmup": warmup}
    stream = torch.cuda.Stream()
    ctxs = [capi.NmiContext(w, h) for _ in range(3)]
    try:
        for c in ctxs:
            c.set_stream(stream.cuda_stream)
        ctxs[1].set_option(ctxs[1].OPT_SPLIT, 0)
        with torch.cuda.stream(stream):
            ws, wm = ctxs[0].warp_stack_masked(frame, Ms)
            ctxs[0].synchronize()
            calls = {
                "masked_pixel_ranges": (ctxs[0], lambda: ctxs[0].search_grid_masked(rs, ws, wm)),
                "masked_grid_kernel": (ctxs[1], lambda: ctxs[1].search_grid_masked(rs, ws, wm)),
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
            assert res["masked_pixel_ranges"] == res["masked_grid_kernel"], res
            out["masked_ranges_over_grid"] = out["masked_pixel_ranges_us"][0] / out["masked_grid_kernel_us"][0]
            out["masked_ranges_over_unmasked_ranges"] = out["masked_pixel_ranges_us"][0] / out["unmasked_pixel_ranges_us"][0]
            out["healed"] = ctxs[0].pix_status()["healed"]
            out["mask_valid_fraction"] = [round(float(n) / (w * h), 4) for n in ctxs[0].mask_counts(Wn)]
    finally:
        for c in ctxs:
            c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    out = {"level": level_part(args.iters, args.warmup), "search81": search_part(args.iters, args.warmup),
           "note": "(median, mean) in us; level: host wall time of nmi_level_run; search81: scoring launches (nmi_set_profiling)"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
