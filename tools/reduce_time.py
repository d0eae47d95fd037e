"""Full-size camera frames timing (nmi_reduce_frame, nmi_level_set_frame_reduction, nmi_stream_set_frame_reduction).  Prints one
JSON line.

1. Kernels, for the profiler: `--rounds` rounds of `--iters` ALTERNATED calls of nmi_reduce_frame (1920x1080 RGB -> 960x540, and
   3840x2160 BGRA -> 960x540) and of nmi_gray_frame on the same sources at full size (nmi_gray_kernel<3,0> / <4,2>: the same input
   bytes, four and sixteen times the output).  The host wall time of the synchronised calls is reported as an upper bound;
   per-kernel times come from rocprofv3 (tools/summarize_reduce_trace.py splits each kernel's dispatches into the rounds).
2. A captured 27 x 27 level at 960x540 on tools/color_time.py's cloud -- plain, masked (hood frame mask) and distorted (barrel
   lens) -- fed a ready 960x540 grey frame, against the same level fed the 1920x1080 RGB frame through
   nmi_level_set_frame_reduction, against the same level run at 1920x1080 on the grey full-size frame (what a caller without the
   reduction can do on the device), replayed ALTERNATELY; host wall time of each nmi_level_run.
3. A keyframe stream at 960x540, 27 views x 27 warps: per keyframe (frame + search, waited for), search-size grey host frames
   against full-size pitched RGB host frames (1920x1080 in rows of 5888 bytes).

Per-kernel times: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/reduce_time.py --part kernel
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if d not in sys.path:
        sys.path.insert(0, d)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbslam2_nmi_amd as nmi  # noqa: E402
from color_time import BARREL, level_scene, med, timed  # noqa: E402
from helpers import color_np as cnp  # noqa: E402
from orbslam2_nmi_amd import capi, hostapi as H, synthetic as sy  # noqa: E402

SEARCH = (960, 540)
KERNEL_CASES = [("1920x1080_rgb_f2", 2, cnp.RGB), ("3840x2160_bgra_f4", 4, cnp.BGRA)]


def kernel_part(iters, warmup, rounds):
    w, h = SEARCH
    out = {"search": [w, h], "iters": iters, "rounds": rounds, "warmup": warmup}
    for name, f, fmt in KERNEL_CASES:
        fw, fh = f * w, f * h
        img = cnp.colorize(sy.camera_frame(sy.scene(fw, fh, 5), 6), 1)
        src = torch.from_numpy(cnp.pack(img, fmt)).cuda()
        with nmi.NmiContext(w, h) as small, nmi.NmiContext(fw, fh) as full:
            g_small = torch.empty((h, w), dtype=torch.uint8, device="cuda")
            g_full = torch.empty((fh, fw), dtype=torch.uint8, device="cuda")
            for _ in range(warmup):
                small.reduce_frame(src, fmt, f, out=g_small)
                full.gray_frame(src, fmt, out=g_full)
            red_rounds, gray_rounds = [], []
            for _ in range(rounds):
                tr, tg = [], []
                for _ in range(iters):
                    t0 = time.perf_counter()
                    small.reduce_frame(src, fmt, f, out=g_small)
                    t1 = time.perf_counter()
                    full.gray_frame(src, fmt, out=g_full)
                    t2 = time.perf_counter()
                    tr.append((t1 - t0) * 1e6)
                    tg.append((t2 - t1) * 1e6)
                red_rounds.append(round(float(np.median(tr)), 2))
                gray_rounds.append(round(float(np.median(tg)), 2))
            out[name] = {"reduce_call_us_round_medians": red_rounds, "gray_full_size_call_us_round_medians": gray_rounds}
    return out


def level_part(iters, warmup):
    w, h = SEARCH
    f = 2
    fw, fh = f * w, f * h
    K, rp, xyz, red = level_scene(w, h)
    full_cfg = dict(fx=K[0, 0] * f, fy=K[1, 1] * f, cx=f * (K[0, 2] + 0.5) - 0.5, cy=f * (K[1, 2] + 0.5) - 0.5)
    Kf = np.array([[full_cfg["fx"], 0, full_cfg["cx"]], [0, full_cfg["fy"], full_cfg["cy"]], [0, 0, 1.0]])
    rpf = capi.RenderParams(near_plane=5.0, far_plane=30.0, point_size=3.0 * f, **full_cfg)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    dx, dr = torch.from_numpy(xyz).cuda(), torch.from_numpy(red).cuda()
    out = {"search": [w, h], "camera": [fw, fh], "grid": [27, 27], "points": int(xyz.shape[0]), "iters": iters, "warmup": warmup}
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, 1] = [0, -1, 0]
    pos, look, up = Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]
    g = H.SearchKernel.make([3] * 6, [0.2, 0.2, 0.5, 0.02, 0.02, 0.05])
    cells = [(sx, sy_, sz) for sz in range(3) for sy_ in range(3) for sx in range(3)]
    with nmi.NmiContext(w, h) as ctx, nmi.NmiContext(fw, fh) as big:
        ctx.set_stream(st.cuda_stream)
        big.set_stream(st.cuda_stream)
        mvps = np.stack([capi.render_mvp(rp, pos, look, up, H.calculate_translation(Twc, g, *c)) for c in cells])
        mvps_f = np.stack([capi.render_mvp(rpf, pos, look, up, H.calculate_translation(Twc, g, *c)) for c in cells])
        homs = capi.warp_homographies(K, (3, 3, 3), tuple(g.step[3:6]))
        homs_f = capi.warp_homographies(Kf, (3, 3, 3), tuple(g.step[3:6]))
        # the camera's frame: the map seen at full size, grey and coloured; the ready search-size frame is its reduction
        shot = torch.flip(big.render_points(dx, torch.sqrt(dr), capi.render_mvp(rpf, pos, look, up, (0, 0, 0))[None], 3.0 * f)[0], dims=[0]).contiguous()
        torch.cuda.synchronize()
        rgb = torch.from_numpy(cnp.pack(cnp.colorize(shot.cpu().numpy(), 1), cnp.RGB)).cuda()
        ready = ctx.reduce_frame(rgb, cnp.RGB, f)
        grey_full = big.gray_frame(rgb, cnp.RGB)
        hood = torch.ones((h, w), dtype=torch.uint8, device="cuda")
        hood[h - h // 6:] = 0
        hood_f = torch.ones((fh, fw), dtype=torch.uint8, device="cuda")
        hood_f[fh - fh // 6:] = 0
        for mode in ("plain", "masked", "distorted"):
            small = nmi.NmiLevel(ctx, dx, dr, ready, 27, 27, 3.0)
            fed = nmi.NmiLevel(ctx, dx, dr, rgb, 27, 27, 3.0)
            fed.set_frame_reduction(f, cnp.RGB, 0)
            large = nmi.NmiLevel(big, dx, dr, grey_full, 27, 27, 3.0 * f)
            if mode == "masked":
                small.set_masks(True, hood), fed.set_masks(True, hood), large.set_masks(True, hood_f)
            if mode == "distorted":
                small.set_distortion(K, BARREL), fed.set_distortion(K, BARREL), large.set_distortion(Kf, BARREL)
            runs = [small.bind(mvps, homs), fed.bind(mvps, homs), large.bind(mvps_f, homs_f)]
            assert runs[0]() == runs[1]()              # the fed level is the ready level
            for _ in range(warmup):
                for r in runs:
                    r()
            ts = [[], [], []]
            for _ in range(iters):
                for k, r in enumerate(runs):
                    t0 = time.perf_counter()
                    r()
                    ts[k].append((time.perf_counter() - t0) * 1e6)
            out[mode] = {"ready_grey_level_us": med(ts[0]), "full_size_rgb_level_us": med(ts[1]), "level_at_full_size_us": med(ts[2]),
                         "added_us": round(med(ts[1])[0] - med(ts[0])[0], 2)}
            for lv in (small, fed, large):
                lv.close()
    torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def stream_part(iters, warmup):
    w, h = SEARCH
    f, pitch = 2, 5888
    K = sy.intrinsics(w, h)
    B = sy.scene(w, h, 5)
    F = sy.camera_frame(B, 6)
    rs = sy.render_stack(B, (3, 3, 3), shift_px=2, zoom_step=0.02)
    Ms = capi.warp_homographies(K, (3, 3, 3), (0.02, 0.02, 0.05))
    big = np.kron(F, np.ones((f, f), np.uint8))
    C = torch.from_numpy(cnp.pack(cnp.colorize(big, 1), cnp.RGB, pitch)).pin_memory()
    G = torch.from_numpy(np.ascontiguousarray(F)).pin_memory()
    R = torch.from_numpy(np.ascontiguousarray(rs)).pin_memory()
    out = {"search": [w, h], "grid": [27, 27], "camera": [f * w, f * h], "rgb_pitch": pitch}
    with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, 27, 27, depth=2) as grey, nmi.NmiStream(ctx, 27, 27, depth=2) as fed:
        fed.set_frame_reduction(f, cnp.RGB, pitch)
        tg = timed(lambda: grey.wait(grey.submit(R, G, Ms)), iters, warmup)
        tc = timed(lambda: fed.wait(fed.submit(R, C, Ms)), iters, warmup)
    out["grey_keyframe_us"] = tg
    out["full_size_rgb_keyframe_us"] = tc
    out["added_us"] = round(tc[0] - tg[0], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--part", choices=["all", "kernel", "level", "stream"], default="all")
    a = ap.parse_args()
    nmi.load_library()
    res = {}
    if a.part in ("all", "kernel"):
        res["kernel"] = kernel_part(a.iters, a.warmup, a.rounds)
    if a.part in ("all", "level"):
        res["level"] = level_part(a.iters, a.warmup)
    if a.part in ("all", "stream"):
        res["stream"] = stream_part(a.iters, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
