"""Lens undistortion timing (nmi_undistort_frame, nmi_level_set_distortion).  Prints one JSON line.

1. The undistortion kernel alone at 640x480 and 848x480, with and without the output mask (and with a raw mask), barrel
   coefficients of a wide-angle camera: host wall time of a synchronised call (upper bound; per-kernel times come from the
   profiler).
2. A captured 27 x 27 level at 848x480 on tools/masked_level_time.py's cloud -- plain, masked (border masks only) and masked
   with a hood frame mask: the same level without and with distortion, replayed ALTERNATELY in the same loop, host wall time
   of each nmi_level_run.  (A distorted masked level always has a frame mask, the undistorted one; "masked_hood" compares it
   with a level that has one too.)

Per-kernel times: run it under rocprofv3 --kernel-trace --stats -- python tools/undistort_time.py --iters 200
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

BARREL = (-0.28, 0.074, 0.0, 0.0, 0.0)


def med(ts):
    return float(np.median(ts)), float(np.mean(ts))


def kernel_part(iters, warmup):
    out = {}
    for w, h in ((640, 480), (848, 480)):
        K = sy.intrinsics(w, h)
        raw = torch.from_numpy(sy.camera_frame(sy.scene(w, h, 5), 6)).cuda()
        rmask = torch.ones((h, w), dtype=torch.uint8, device="cuda")
        rmask[h - h // 6:] = 0
        with nmi.NmiContext(w, h) as ctx:
            fr = torch.empty((h, w), dtype=torch.uint8, device="cuda")
            fm = torch.empty((h, w), dtype=torch.uint8, device="cuda")
            cases = {"frame": dict(out_mask=False), "frame_and_mask": dict(out_mask=fm), "frame_and_mask_raw_mask": dict(out_mask=fm, raw_mask=rmask)}
            for name, kw in cases.items():
                for _ in range(warmup):
                    ctx.undistort_frame(raw, K, BARREL, out=fr, **kw)
                ts = []
                for _ in range(iters):
                    t0 = time.perf_counter()
                    ctx.undistort_frame(raw, K, BARREL, out=fr, **kw)
                    ts.append((time.perf_counter() - t0) * 1e6)
                out[f"undistort_{w}x{h}_{name}_call_us"] = med(ts)
            out[f"valid_fraction_{w}x{h}"] = round(float(fm.float().mean()), 4)
    return out


def level_part(iters, warmup):
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
        hood = torch.ones((h, w), dtype=torch.uint8, device="cuda")
        hood[h - h // 6:] = 0
        for mode in ("plain", "masked", "masked_hood"):
            plain = nmi.NmiLevel(ctx, dx, dr, frame, 27, 27, 3.0)
            dist = nmi.NmiLevel(ctx, dx, dr, frame, 27, 27, 3.0)
            if mode != "plain":
                fm = hood if mode == "masked_hood" else None
                plain.set_masks(True, fm)
                dist.set_masks(True, fm)
            dist.set_distortion(Kl, BARREL)
            run_p, run_d = plain.bind(mvps, homs), dist.bind(mvps, homs)
            for _ in range(warmup):
                run_p(), run_d()
            tp, td = [], []
            for _ in range(iters):
                t0 = time.perf_counter()
                run_p()
                t1 = time.perf_counter()
                run_d()
                t2 = time.perf_counter()
                tp.append((t1 - t0) * 1e6)
                td.append((t2 - t1) * 1e6)
            tag = "" if mode == "plain" else mode + "_"
            out[tag + "level_us"] = med(tp)
            out[tag + "distorted_level_us"] = med(td)
            out[tag + "added_us"] = out[tag + "distorted_level_us"][0] - out[tag + "level_us"][0]
            plain.close()
            dist.close()
    torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    nmi.load_library()
    res = {"kernel": kernel_part(a.iters, a.warmup), "level": level_part(a.iters, a.warmup)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
