"""Kernel time of the fisheye undistortion beside the radial-tangential one (profiles/fisheye/README.md).

Run under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o fisheye -- python tools/fisheye_time.py --iters 200
    python tools/fisheye_time.py --summarize OUT/.../fisheye_kernel_trace.csv --iters 200

The run makes, on one 848x480 frame, four groups of 2 x iters dispatches of nmi_undistort_kernel, the two lens models
alternated call by call: a grey frame through nmi_undistort_frame / nmi_undistort_frame_fisheye without and with masks, then a
BGR frame through a 1 x 1 level (the fused colour node) plain and masked.  The summary tells the instantiations apart by
their names and the groups by their order, drops each group's first tenth as warm-up and prints medians in microseconds.
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H = 848, 480
RADTAN = (-0.28, 0.074, 0.0002, 0.00002, 0.0)        # a wide-angle MAV camera
FISHEYE = (0.00348, 0.000715, -0.00205, 0.000203)    # a TUM-VI camera


def run(iters):
    import numpy as np
    import torch

    import orbslam2_nmi_amd as nmi
    from orbslam2_nmi_amd import capi
    from orbslam2_nmi_amd import synthetic as sy

    nmi.load_library()
    K = sy.intrinsics(W, H)
    K_raw = K.copy()                  # the fisheye's own camera: a longer focal length, as a frame undistorted onto K would have
    K_raw[0, 0] /= 0.6
    K_raw[1, 1] /= 0.6
    gray = sy.camera_frame(sy.scene(W, H, 3), 4)
    rng = np.random.default_rng(5)
    bgr = np.clip(gray[..., None].astype(int) + rng.integers(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)
    raw_mask = torch.from_numpy((rng.random((H, W)) < 0.9).astype(np.uint8)).cuda()
    with nmi.NmiContext(W, H) as ctx:
        raw = torch.from_numpy(gray).cuda()
        out = torch.empty_like(raw)
        out_mask = torch.empty_like(raw)
        for masked in (False, True):
            kw = dict(raw_mask=raw_mask, out=out, out_mask=out_mask) if masked else dict(out=out, out_mask=False)
            for _ in range(iters):
                ctx.undistort_frame(raw, K, RADTAN, **kw)
                ctx.undistort_frame_fisheye(raw, K, K_raw, FISHEYE, **kw)
        xyz = torch.from_numpy((rng.random((500, 3)) * [8, 6, 0] + [-4, -3, 10]).astype(np.float32)).cuda()
        red = torch.from_numpy(rng.random(500).astype(np.float32)).cuda()
        rp = capi.RenderParams(K[0, 0], K[1, 1], K[0, 2], K[1, 2], 5.0, 30.0, 3.0)
        mvps = capi.render_mvp(rp, (0, 0, 0), (0, 0, 1), (0, -1, 0), (0, 0, 0))[None]
        Ms = np.eye(3)[None]
        frame = torch.from_numpy(bgr).cuda()
        with nmi.NmiLevel(ctx, xyz, red, frame, 1, 1, 3.0) as lr, nmi.NmiLevel(ctx, xyz, red, frame, 1, 1, 3.0) as lf:
            for lv in (lr, lf):
                lv.set_frame_format(capi.FRAME_BGR, 0)
            lr.set_distortion(K, RADTAN)
            lf.set_distortion_fisheye(K, K_raw, FISHEYE)
            for masked in (False, True):
                for lv in (lr, lf):
                    lv.set_masks(masked, raw_mask if masked else None)
                for _ in range(iters):
                    lr.run(mvps, Ms)
                    lf.run(mvps, Ms)
        ctx.synchronize()


def summarize(path, iters):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "nmi_undistort_kernel" not in name:
                continue
            m = re.search(r"Taps(?:<\d, \d>)?, (\d)>\(", name) or re.search(r"ELi(\d)EEEv", name)   # the Model parameter
            taps = "bgr" if "ColorTaps" in name else "grey"
            rows.append((int(r["Start_Timestamp"]), taps, "fisheye" if m and m.group(1) == "1" else "radtan",
                         (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    out = {}
    for taps in ("grey", "bgr"):
        for model in ("radtan", "fisheye"):
            us = [d for _, t, m, d in rows if t == taps and m == model]
            if len(us) != 2 * iters:
                sys.exit(f"{taps} {model}: {len(us)} dispatches, expected {2 * iters}")
            for label, part in (("no mask", us[:iters]), ("mask", us[iters:])):
                kept = part[iters // 10:]
                out[f"{taps}, {label}, {model}"] = {"median_us": round(statistics.median(kept), 2), "min_us": round(min(kept), 2),
                                                   "max_us": round(max(kept), 2), "n": len(kept)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--summarize", metavar="KERNEL_TRACE_CSV")
    a = ap.parse_args()
    summarize(a.summarize, a.iters) if a.summarize else run(a.iters)
