"""Raw sensor frames timing (NMI_FRAME_YUYV / _UYVY / _BAYER_* through nmi_gray_frame, nmi_level_set_frame_format and
nmi_stream_set_frame_format), after tools/color_time.py.  Prints one JSON line.

1. kernel: nmi_gray_frame alone on RGB and on each raw format at 848x480 and 1241x376 (dense rows), in --repeats passes, and at
   848x480 the two-node chain nmi_gray_frame (Bayer) -> nmi_undistort_frame: host wall time of a synchronised call (an upper
   bound; kernel times come from the profiler, tools/summarize_sensor_trace.py, which also splits each kernel's dispatches into
   the passes to give the spread of its median).  --rgb-only keeps to the RGB conversion, which a library built from an earlier
   commit runs too (NMI_HIP_LIBRARY points the loader at it): the same session's bar for the new kernels.
2. level: a captured 27 x 27 level at 848x480 on tools/color_time.py's cloud, plain and distorted (barrel lens; a raw level's
   node is the fused one, each bilinear tap converted): a grey level and the same level on a Bayer mosaic or a YUYV frame,
   replayed ALTERNATELY, host wall time of each nmi_level_run.
3. stream: a keyframe stream at 848x480, 27 views x 27 warps, per keyframe (frame + search, waited for): grey host frames, RGB
   in rows of 2560 bytes, a Bayer mosaic and YUYV (both dense), in turns.

Kernel times: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/sensor_time.py --iters 100
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import orbslam2_nmi_amd as nmi  # noqa: E402
from color_time import BARREL, level_scene, med, timed  # noqa: E402
from helpers import color_np as cnp  # noqa: E402
from helpers import sensor_np as snp  # noqa: E402
from orbslam2_nmi_amd import capi, hostapi as H, synthetic as sy  # noqa: E402


def raw(rgb, gray, fmt, pitch=0):
    """The frame in fmt: RGB packed, a mosaic of the colour image, or the grey frame as luma."""
    if fmt == cnp.RGB:
        return cnp.pack(rgb, fmt, pitch)
    return snp.pack(snp.mosaic(rgb, fmt) if snp.is_bayer(fmt) else gray, fmt, pitch)


def kernel_part(iters, warmup, repeats, rgb_only):
    fmts = {"rgb": cnp.RGB} if rgb_only else {"rgb": cnp.RGB, **snp.FORMATS}
    out = {"repeats": repeats}
    for w, h in ((848, 480), (1241, 376)):
        gray = sy.camera_frame(sy.scene(w, h, 5), 6)
        rgb = cnp.colorize(gray, 1)
        with nmi.NmiContext(w, h) as ctx:
            g = torch.empty((h, w), dtype=torch.uint8, device="cuda")
            srcs = {name: torch.from_numpy(raw(rgb, gray, fmt)).cuda() for name, fmt in fmts.items()}
            for name, fmt in fmts.items():
                out[f"gray_{w}x{h}_{name}_call_us"] = []
            for _ in range(repeats):
                for name, fmt in fmts.items():
                    out[f"gray_{w}x{h}_{name}_call_us"].append(timed(lambda: ctx.gray_frame(srcs[name], fmt, out=g), iters, warmup)[0])
            if w == 848 and not rgb_only:
                K = sy.intrinsics(w, h)
                ud = torch.empty((h, w), dtype=torch.uint8, device="cuda")

                def chain():
                    ctx.gray_frame(srcs["rggb"], snp.RGGB, out=g, sync=False)
                    ctx.undistort_frame(g, K, BARREL, out=ud, out_mask=False)
                out[f"chain_{w}x{h}_rggb_gray_then_undistort_call_us"] = timed(chain, iters, warmup)
    return out


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
        fnp_ = frame.cpu().numpy()
        rgb = cnp.colorize(fnp_, 1)
        for mode in ("plain", "distorted"):
            res = {}
            for name, fmt in (("rggb", snp.RGGB), ("yuyv", snp.YUYV)):
                src = torch.from_numpy(raw(rgb, fnp_, fmt)).cuda()
                grey = nmi.NmiLevel(ctx, dx, dr, frame, 27, 27, 3.0)
                col = nmi.NmiLevel(ctx, dx, dr, src, 27, 27, 3.0)
                col.set_frame_format(fmt, 0)
                if mode == "distorted":
                    grey.set_distortion(Kl, BARREL)
                    col.set_distortion(Kl, BARREL)
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
                res[name] = {"grey_level_us": med(tg), "raw_level_us": med(tc), "added_us": round(med(tc)[0] - med(tg)[0], 2)}
                grey.close()
                col.close()
            out[mode] = res
    torch.cuda.set_stream(torch.cuda.default_stream())
    return out


def stream_part(iters, warmup, rounds=4):
    w, h = 848, 480
    K = sy.intrinsics(w, h)
    B = sy.scene(w, h, 5)
    F = sy.camera_frame(B, 6)
    C = cnp.colorize(F, 1)
    rs = sy.render_stack(B, (3, 3, 3), shift_px=2, zoom_step=0.02)
    Ms = capi.warp_homographies(K, (3, 3, 3), (0.02, 0.02, 0.05))
    R = torch.from_numpy(np.ascontiguousarray(rs)).pin_memory()
    layouts = {"grey": (cnp.GRAY, 0), "rgb": (cnp.RGB, 2560), "bayer": (snp.RGGB, 0), "yuyv": (snp.YUYV, 0)}
    out = {"shape": [w, h], "grid": [27, 27], "rgb_pitch": 2560, "rounds": rounds}
    for lens in (None, BARREL):
        tag = "barrel_" if lens is not None else ""
        with nmi.NmiContext(w, h) as ctx:
            streams, frames, ts = {}, {}, {}
            for name, (fmt, pitch) in layouts.items():
                s = nmi.NmiStream(ctx, 27, 27, depth=2)
                s.set_frame_format(fmt, pitch)
                if lens is not None:
                    s.set_distortion(K, lens)
                streams[name] = s
                frames[name] = torch.from_numpy(np.ascontiguousarray(F) if fmt == cnp.GRAY else raw(C, F, fmt, pitch)).pin_memory()
                ts[name] = []
            for _ in range(rounds):  # the four in turns, so that a drift of the host shows in all of them
                for name, s in streams.items():
                    ts[name].append(timed(lambda: s.wait(s.submit(R, frames[name], Ms)), iters // rounds, warmup)[0])
            for name, s in streams.items():
                out[f"{tag}{name}_keyframe_us"] = {"median_of_rounds": round(float(np.median(ts[name])), 2), "rounds": ts[name]}
                s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rgb-only", action="store_true")
    ap.add_argument("--part", choices=["kernel", "level", "stream", "all"], default="all")
    a = ap.parse_args()
    nmi.load_library()
    res = {}
    if a.part in ("kernel", "all"):
        res["kernel"] = kernel_part(a.iters, a.warmup, a.repeats, a.rgb_only)
    if a.part in ("level", "all") and not a.rgb_only:
        res["level"] = level_part(a.iters, a.warmup)
    if a.part in ("stream", "all") and not a.rgb_only:
        res["stream"] = stream_part(a.iters, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
