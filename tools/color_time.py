"""Colour and pitched camera frames timing (nmi_gray_frame, nmi_level_set_frame_format, nmi_stream_set_frame_format).  Prints one
JSON line.

1. nmi_gray_frame alone per format at 848x480 and 1241x376 (dense rows), and the two-node chain nmi_gray_frame ->
   nmi_undistort_frame at 848x480: host wall time of a synchronised call (upper bound; per-kernel times come from the profiler).
2. A captured 27 x 27 level at 848x480 on tools/undistort_time.py's cloud -- plain, masked (hood frame mask) and distorted (barrel
   lens) -- a grey level and the same level on each colour format, replayed ALTERNATELY, host wall time of each nmi_level_run.
   The distorted coloured level is the fused node (convert + undistort); "chain_estimate_us" adds the plain coloured level's
   extra time (the conversion node) to the grey distorted level's: the replay a two-node chain would give.
3. A keyframe stream at 848x480, 27 views x 27 warps: per keyframe (frame + search, waited for), grey host frames against
   pitched RGB host frames (rows of 2560 bytes), and both with the barrel lens.

Per-kernel times: run it under rocprofv3 --kernel-trace --stats -- python tools/color_time.py --iters 200
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TESTS = os.path.join(ROOT, "tests")
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbslam2_nmi_amd as nmi  # noqa: E402
from helpers import color_np as cnp  # noqa: E402
from orbslam2_nmi_amd import capi, hostapi as H, synthetic as sy  # noqa: E402

BARREL = (-0.28, 0.074, 0.0, 0.0, 0.0)
NAMES = {cnp.BGR: "bgr", cnp.RGB: "rgb", cnp.BGRA: "bgra", cnp.RGBA: "rgba"}


def med(ts):
    return round(float(np.median(ts)), 2), round(float(np.mean(ts)), 2)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return med(ts)


def kernel_part(iters, warmup):
    out = {}
    for w, h in ((848, 480), (1241, 376)):
        img = cnp.colorize(sy.camera_frame(sy.scene(w, h, 5), 6), 1)
        with nmi.NmiContext(w, h) as ctx:
            g = torch.empty((h, w), dtype=torch.uint8, device="cuda")
            for fmt, name in NAMES.items():
                src = torch.from_numpy(cnp.pack(img, fmt)).cuda()
                out[f"gray_{w}x{h}_{name}_call_us"] = timed(lambda: ctx.gray_frame(src, fmt, out=g), iters, warmup)
            if w == 848:
                K = sy.intrinsics(w, h)
                src = torch.from_numpy(cnp.pack(img, cnp.RGB)).cuda()
                ud = torch.empty((h, w), dtype=torch.uint8, device="cuda")

                def chain():
                    ctx.gray_frame(src, cnp.RGB, out=g, sync=False)
                    ctx.undistort_frame(g, K, BARREL, out=ud, out_mask=False)
                out[f"chain_{w}x{h}_rgb_gray_then_undistort_call_us"] = timed(chain, iters, warmup)
    return out


def level_scene(w, h):
    K = sy.intrinsics(w, h)
    rp = capi.RenderParams(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], near_plane=5.0, far_plane=30.0, point_size=3.0)
    B = sy.scene(2 * w, 2 * h, 77)
    nu, nv = int(3 * w * 0.9), int(3 * h * 0.9)
    uu, vv = np.meshgrid(np.linspace(-w, 2 * w, nu), np.linspace(-h, 2 * h, nv))
    xyz = np.stack([(uu - rp.cx) / rp.fx * 10.0, (vv - rp.cy) / rp.fy * 10.0, np.full_like(uu, 10.0)], -1).reshape(-1, 3).astype(np.float32)
    red = (B[np.clip(((vv + h) / 3 * 2).astype(int), 0, 2 * h - 1), np.clip(((uu + w) / 3 * 2).astype(int), 0, 2 * w - 1)].astype(np.float32)
           / np.float32(256)).reshape(-1)
    return K, rp, xyz, red


def level_part(iters, warmup):
    w, h = 848, 480
    K, rp, xyz, red = level_scene(w, h)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    dx, dr = torch.from_numpy(xyz).cuda(), torch.from_numpy(red).cuda()
    out = {"shape": [w, h], "grid": [27, 27], "points": int(xyz.shape[0]), "iters": iters, "warmup": warmup}
    Kl = np.array([[rp.fx, 0, rp.cx], [0, rp.fy, rp.cy], [0, 0, 1.0]])
    with nmi.NmiContext(w, h) as ctx:
        ctx.set_stream(st.cuda_stream)
        Twc = np.eye(4, dtype=np.float32)
        Twc[:3, 1] = [0, -1, 0]
        pos, look, up = Twc[:3, 3], Twc[:3, 3] + Twc[:3, 2], Twc[:3, 1]
        g = H.SearchKernel.make([3] * 6, [0.2, 0.2, 0.5, 0.02, 0.02, 0.05])
        cells = [(sx, sy_, sz) for sz in range(3) for sy_ in range(3) for sx in range(3)]
        mvps = np.stack([capi.render_mvp(rp, pos, look, up, H.calculate_translation(Twc, g, *c)) for c in cells])
        homs = capi.warp_homographies(K, (3, 3, 3), tuple(g.step[3:6]))
        frame = torch.flip(ctx.render_points(dx, torch.sqrt(dr), capi.render_mvp(rp, pos, look, up, (0, 0, 0))[None], 3.0)[0], dims=[0]).contiguous()
        torch.cuda.synchronize()
        rgb = cnp.colorize(frame.cpu().numpy(), 1)
        srcs = {fmt: torch.from_numpy(cnp.pack(rgb, fmt)).cuda() for fmt in NAMES}
        hood = torch.ones((h, w), dtype=torch.uint8, device="cuda")
        hood[h - h // 6:] = 0
        for mode in ("plain", "masked", "distorted"):
            res = {}
            for fmt, name in NAMES.items():
                grey = nmi.NmiLevel(ctx, dx, dr, frame, 27, 27, 3.0)
                col = nmi.NmiLevel(ctx, dx, dr, srcs[fmt], 27, 27, 3.0)
                col.set_frame_format(fmt, 0)
                for lv in (grey, col):
                    if mode == "masked":
                        lv.set_masks(True, hood)
                    if mode == "distorted":
                        lv.set_distortion(Kl, BARREL)
                run_g, run_c = grey.bind(mvps, homs), col.bind(mvps, homs)
                for _ in range(warmup):
                    run_g(), run_c()
                tg, tc = [], []
                for _ in range(iters):
                    t0 = time.perf_counter()
                    run_g()
                    t1 = time.perf_counter()
                    run_c()
                    t2 = time.perf_counter()
                    tg.append((t1 - t0) * 1e6)
                    tc.append((t2 - t1) * 1e6)
                res[name] = {"grey_level_us": med(tg), "color_level_us": med(tc), "added_us": round(med(tc)[0] - med(tg)[0], 2)}
                grey.close()
                col.close()
            out[mode] = res
        out["distorted_fused_vs_chain_estimate"] = {
            name: {"fused_added_us": out["distorted"][name]["added_us"], "chain_estimate_added_us": out["plain"][name]["added_us"]}
            for name in NAMES.values()}
    torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def stream_part(iters, warmup):
    w, h = 848, 480
    K = sy.intrinsics(w, h)
    B = sy.scene(w, h, 5)
    F = sy.camera_frame(B, 6)
    rs = sy.render_stack(B, (3, 3, 3), shift_px=2, zoom_step=0.02)
    Ms = capi.warp_homographies(K, (3, 3, 3), (0.02, 0.02, 0.05))
    pitch = 2560
    C = torch.from_numpy(cnp.pack(cnp.colorize(F, 1), cnp.RGB, pitch)).pin_memory()
    G = torch.from_numpy(np.ascontiguousarray(F)).pin_memory()
    R = torch.from_numpy(np.ascontiguousarray(rs)).pin_memory()
    out = {"shape": [w, h], "grid": [27, 27], "rgb_pitch": pitch}
    for lens in (None, BARREL):
        with nmi.NmiContext(w, h) as ctx, nmi.NmiStream(ctx, 27, 27, depth=2) as grey, nmi.NmiStream(ctx, 27, 27, depth=2) as col:
            col.set_frame_format(cnp.RGB, pitch)
            if lens is not None:
                grey.set_distortion(K, lens)
                col.set_distortion(K, lens)
            tg = timed(lambda: grey.wait(grey.submit(R, G, Ms)), iters, warmup)
            tc = timed(lambda: col.wait(col.submit(R, C, Ms)), iters, warmup)
        tag = "barrel_" if lens is not None else ""
        out[tag + "grey_keyframe_us"] = tg
        out[tag + "rgb_keyframe_us"] = tc
        out[tag + "added_us"] = round(tc[0] - tg[0], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    nmi.load_library()
    res = {"kernel": kernel_part(a.iters, a.warmup), "level": level_part(a.iters, a.warmup), "stream": stream_part(a.iters, a.warmup)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
